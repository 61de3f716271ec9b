"""Train the verifier (scripts/train.py's command line; one GPU, or --gpus N of one node data-parallel):

    python -m salve_amd.train --config <reference yaml> [--gpus N [--dist-backend {nccl,gloo}] [--dist-timeout S] [--sync-bn]] [--epochs N] [--batch-size B] [--data-root DIR]
                              [--layout-data-root DIR] [--seed S] [--init-ckpt CKPT] [--out DIR] [--precision {fp32,bf16}]
                              [--norm {torch,hip}] [--optim {torch,hip}] [--head {torch,hip}] [--decode {host,device}]
                              [--decode-entropy {image,lanes}] [--decode-read-ahead] [--photometric device]
                              [--render-from DIR [--identity {kept,batch}] [--resident-panos N [--prefetch]] [--jpeg-quality Q]]

Writes `train_ckpt.pth` (the reference's keys) and `results-{cfg_stem}.json` into --out (default: the config's
model_save_dirpath / a time stamp, as the reference does).  --precision bf16 opts into mixed precision (bf16 activations and
convolutions, fp32 master weights, gradients and checkpoint); the default fp32 is the reference's.  --norm hip opts into the HIP
BatchNorm with fused ReLU and residual add (same checkpoint); the default is torch's BatchNorm.  --optim hip opts into HipAdam
(salve_amd/optim.py): torch.optim.Adam's update in one HIP launch per step, which with --precision bf16 also writes the
convolution weights' bf16 copies; the checkpoint's "optimizer" entry keeps torch's format.  --head hip opts into the fused HIP
classifier head (average pool, fc, softmax, cross-entropy, accuracy counts): loss and accuracy are accumulated on the device and
read once per pass, so the host never waits for the device between batches; the default is torch's head.  See salve_amd/training.py.
--decode device (the rendered dataset on disk; not with --render-from) reads each batch's JPEG tiles with a thread pool, decodes them on
the GPU in one call and makes the batch with one tile launch (salve_amd/train_files.py); the default, host, decodes every tile with
Pillow in the DataLoader.  The batches are the same bits.  --decode-entropy lanes (with --decode device) takes the lane-parallel
entropy stage, which also decodes tiles written with restart intervals on the GPU; the same bits again.
--decode-read-ahead (with --decode device) reads the next two batches' files and decodes the next batch on a second stream while the
current batch trains: the same bits once more, one more batch of decoded tiles and one more decode workspace on the device.
--render-from DIR trains from panoramas instead of a rendered dataset: DIR holds panos_rgb.npy, panos_depth.npy, train.json and
val.json, the batches are rendered and augmented on the GPU (salve_amd/train_render.py); data_root is not read.
A configuration whose modalities include "layout" also needs DIR/layouts.npz: the layouts are posed and drawn on the GPU.
--identity batch renders the identity images of a batch's second panoramas with the batch instead of keeping one per panorama;
--resident-panos N (which selects --identity batch) memory-maps the two .npy files and keeps a pool of N panoramas on the device,
uploaded as the batches need them: for panorama sets that do not fit in device memory.  N must be at least 2 x batch_size.
--prefetch (with --resident-panos N, N at least 4 x batch_size) uploads the next batch's missing panoramas on a second stream while the
current batch trains: the same batches, the uploads hidden under the step.
--jpeg-quality Q (with --render-from; the reference's files: 75) puts every rendered image through the reference's JPEG round trip on
the GPU before it is tiled: the batches of the rendered dataset on disk, without the files.
--photometric device permits a config with apply_photometric_augmentation: True (refused without it): the reference's PhotometricShift --
ColorJitter(brightness 0.5, contrast 0.5, saturation 0.5, hue 0.05) on every resized train image, each with draws of its own -- runs on
the GPU inside the train-tile call of whichever feed is selected.  With the field False the flag changes nothing.
--gpus N (default 1; at most 16) trains data-parallel on N GPUs of this node (salve_amd/dist_train.py): started without
a launcher, the program starts `python -m torch.distributed.run --nnodes=1 --nproc-per-node=N -m salve_amd.train ...` as a child
process -- before anything touches a GPU -- and relays its exit code; a node that shows fewer than N GPUs is refused in one line.
Every rank trains its rows of each batch (the batch size must be a multiple of N), the gradients are averaged by one all-reduce per
step, rank 0 logs and writes the checkpoint and the results JSON.  Needs --render-from or --decode device.  --dist-backend: nccl
(default: RCCL, a GPU per rank) or gloo (the buffer is reduced on the host).
--sync-bn (with --norm hip; refused without it) makes every BatchNorm of the train pass normalise over the rows of all N ranks
(DESIGN.md 4.26): two small all-gathers per BatchNorm and step, the same running statistics on every rank.  With one rank it changes
nothing.
"""

from __future__ import annotations

import argparse
import logging
import os
import socket
import subprocess
import sys
import time

from salve_amd import training
from salve_amd.training_config import load_training_config


def _self_launch(gpus: int, argv) -> int:
    """`python -m salve_amd.train --gpus N` without a launcher: the N ranks run under torch.distributed.run as a CHILD process (this
    process has not touched the GPU and never will; nothing is exec'ed in place).  Returns the child's exit code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "salve_amd.train"] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, help="a reference config (salve/configs/*.yaml layout)")
    ap.add_argument("--epochs", type=int, default=None, help="override num_epochs")
    ap.add_argument("--batch-size", type=int, default=None, help="override batch_size")
    ap.add_argument("--data-root", default=None, help="override data_root")
    ap.add_argument("--layout-data-root", default=None, help="override layout_data_root")
    ap.add_argument("--seed", type=int, default=0, help="seeds random, numpy, torch and the shuffle order (the reference: 0)")
    ap.add_argument("--init-ckpt", default=None, help="fine-tune: start from this checkpoint's state_dict (strict)")
    ap.add_argument("--out", default=None, help="results directory (default: model_save_dirpath/<time stamp>)")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32",
                    help="fp32 (default, the reference's) or bf16 mixed precision (fp32 master weights and checkpoint)")
    ap.add_argument("--norm", choices=("torch", "hip"), default="torch",
                    help="torch (default: nn.BatchNorm2d) or hip (BatchNorm with fused ReLU and residual add on the HIP kernels)")
    ap.add_argument("--optim", choices=("torch", "hip"), default="torch",
                    help="torch (default: torch.optim.Adam) or hip (the same update in one HIP launch; with bf16 it also writes the weights' bf16 copies)")
    ap.add_argument("--head", default="torch",
                    help="torch (default: avgpool, fc, softmax, cross_entropy) or hip (one fused HIP forward and backward; loss and accuracy stay on the device)")
    ap.add_argument("--decode", choices=("host", "device"), default="host",
                    help="host (default: Pillow decodes each tile in the DataLoader) or device (whole batches of JPEG tiles decoded on the GPU)")
    ap.add_argument("--decode-entropy", choices=("image", "lanes"), default="image",
                    help="--decode device: image (default: one wavefront per tile) or lanes (a lane per 128 bytes of scan; also takes tiles with restart intervals)")
    ap.add_argument("--decode-read-ahead", action="store_true",
                    help="--decode device: read the next batches' tiles and decode the next batch beside the training step (the same batches)")
    ap.add_argument("--render-from", default=None, metavar="DIR",
                    help="render the training batches on the GPU from DIR/panos_rgb.npy, panos_depth.npy, train.json, val.json")
    ap.add_argument("--identity", choices=("kept", "batch"), default=None,
                    help="--render-from: keep one identity image per panorama (kept, the default) or render them with each batch (batch)")
    ap.add_argument("--resident-panos", type=int, default=None, metavar="N",
                    help="--render-from: keep a pool of N panoramas on the device and upload the others as batches need them (selects --identity batch)")
    ap.add_argument("--prefetch", action="store_true",
                    help="--resident-panos: upload the next batch's missing panoramas beside the training step (N at least 4 x batch size)")
    ap.add_argument("--jpeg-quality", type=int, default=None, metavar="Q",
                    help="--render-from: JPEG round trip of every rendered image on the GPU at quality Q (the reference writes its tiles at 75)")
    ap.add_argument("--photometric", choices=("device",), default=None,
                    help="accept apply_photometric_augmentation: True and run the photometric augmentation on the GPU (without it such a config is refused)")
    ap.add_argument("--gpus", type=int, default=1, metavar="N", help="train data-parallel on N GPUs of this node, one process each (default 1)")
    ap.add_argument("--dist-backend", choices=("nccl", "gloo"), default="nccl",
                    help="--gpus: nccl (default: RCCL reduces the gradients on the devices) or gloo (they are reduced on the host)")
    ap.add_argument("--dist-timeout", type=float, default=600, metavar="S", help="--gpus: seconds a collective may wait for the other ranks (default 600)")
    ap.add_argument("--sync-bn", action="store_true",
                    help="--gpus with --norm hip: every BatchNorm normalises over the rows of all ranks, and all ranks keep the same running statistics")
    ap.add_argument("--force-dist", action="store_true", help=argparse.SUPPRESS)   # under a launcher: run the collectives in a world of one too
    argv = sys.argv[1:] if argv is None else list(argv)
    a = ap.parse_args(argv)
    training._check_head(a.head)
    from salve_amd.dist_train import MAX_GPUS

    if a.sync_bn and a.norm != "hip":
        raise SystemExit("--sync-bn synchronises the statistics of the HIP BatchNorm: add --norm hip; nothing was launched")
    if not 1 <= a.gpus <= MAX_GPUS:
        raise SystemExit(f"salve_amd.train: --gpus must be 1 .. {MAX_GPUS}, got {a.gpus}; nothing was launched")
    launched = "WORLD_SIZE" in os.environ
    if not launched and a.gpus > 1:
        import torch

        have = torch.cuda.device_count()   # (does not initialise the GPU)
        if a.gpus > have:
            raise SystemExit(f"salve_amd.train: --gpus {a.gpus} but this node shows {have} GPU(s); nothing was launched")
        if a.render_from is None and a.decode != "device":
            raise SystemExit("--gpus N trains from --render-from DIR or with --decode device: the host DataLoader feed (--decode host) is not sharded")
        raise SystemExit(_self_launch(a.gpus, argv))
    if launched and int(os.environ["WORLD_SIZE"]) != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}")
    if a.gpus > 1 and a.render_from is None and a.decode != "device":
        raise SystemExit("--gpus N trains from --render-from DIR or with --decode device: the host DataLoader feed (--decode host) is not sharded")
    if a.decode_entropy != "image" and a.decode != "device":
        raise SystemExit("--decode-entropy selects the entropy stage of --decode device")
    if a.decode_read_ahead and a.decode != "device":
        raise SystemExit("--decode-read-ahead reads ahead for --decode device")
    if a.decode == "device" and a.render_from is not None:
        raise SystemExit("--decode device reads the rendered dataset on disk: it cannot be combined with --render-from DIR (which reads no tile file)")
    if a.jpeg_quality is not None:
        if a.render_from is None:
            raise SystemExit("--jpeg-quality belongs to --render-from DIR (a rendered dataset on disk already holds JPEG files)")
        if not 1 <= a.jpeg_quality <= 100:
            raise SystemExit(f"--jpeg-quality must be 1 .. 100, got {a.jpeg_quality}")
    if a.render_from is None and (a.identity is not None or a.resident_panos is not None):
        raise SystemExit("--identity and --resident-panos belong to --render-from DIR")
    if a.resident_panos is not None:
        if a.identity == "kept":
            raise SystemExit("--resident-panos keeps no identity image per panorama: it cannot be combined with --identity kept")
        if a.resident_panos <= 0:
            raise SystemExit(f"--resident-panos must be positive, got {a.resident_panos}")
    if a.prefetch:
        if a.identity == "kept":
            raise SystemExit("--prefetch uploads into the --resident-panos pool: it cannot be combined with --identity kept")
        if a.resident_panos is None:
            raise SystemExit("--prefetch belongs to --resident-panos N: without a pool nothing is uploaded per batch")
    identity = a.identity or ("batch" if a.resident_panos is not None else "kept")
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    args = load_training_config(a.config)
    if a.epochs is not None:
        args.num_epochs = a.epochs
    if a.batch_size is not None:
        args.batch_size = a.batch_size
    if a.data_root is not None:
        args.data_root = a.data_root
    if a.layout_data_root is not None:
        args.layout_data_root = a.layout_data_root
    out = a.out or f"{args.model_save_dirpath}/{time.strftime('%Y_%m_%d_%H_%M_%S')}"
    dist = None
    if launched:
        from salve_amd.dist_train import DataParallel

        dist = DataParallel.from_env(a.dist_backend, timeout_s=a.dist_timeout, force=a.force_dist)
    rank, world = (dist.rank, dist.world) if dist is not None else (0, 1)
    if rank == 0:
        logging.info(str(args))
    try:
        results = _train(a, args, out, identity, dist, rank, world)
    finally:
        if dist is not None:
            dist.close()
    if rank == 0:
        logging.info(f"results in {out}: {results}")


def _train(a, args, out: str, identity: str, dist, rank: int, world: int):
    if a.render_from is not None:
        import torch

        from salve_amd import train_render

        rgb, depth, examples = train_render.load_render_dir(a.render_from, mmap=a.resident_panos is not None)
        layouts = train_render.load_render_layouts(a.render_from, len(rgb)) if "layout" in set(args.modalities) else None
        sources = {}
        for split in ("train", "val"):
            src = train_render.RenderedTrainSource(torch.device("cuda", torch.cuda.current_device()), args.modalities, pano_hw=rgb.shape[1:3],
                                                   batch_size=args.batch_size, precision=a.precision, split=split, seed=a.seed,
                                                   resize_hw=(args.resize_h, args.resize_w), crop_hw=(args.train_h, args.train_w),
                                                   identity=identity, resident_panos=a.resident_panos, layouts=layouts, prefetch=a.prefetch,
                                                   jpeg_quality=a.jpeg_quality,
                                                   photometric=a.photometric if args.apply_photometric_augmentation else None,
                                                   rank=rank, world=world)
            if split == "train":
                src.load_panos(rgb, depth)
            else:   # the panoramas (or their pool) and their identity renders are on the device once
                src.share_panos(sources["train"])
            src.set_examples(*examples[split])
            sources[split] = src
        return training.train_rendered(args, sources["train"], sources["val"], out, seed=a.seed, init_ckpt=a.init_ckpt, precision=a.precision,
                                       norm=a.norm, optim=a.optim, head=a.head, jpeg_quality=a.jpeg_quality, photometric=a.photometric, dist=dist,
                                       sync_bn=a.sync_bn)
    return training.train(args, out, seed=a.seed, init_ckpt=a.init_ckpt, precision=a.precision, norm=a.norm, optim=a.optim,
                          head=a.head, decode=a.decode, entropy=a.decode_entropy, read_ahead=a.decode_read_ahead,
                          photometric=a.photometric, dist=dist, sync_bn=a.sync_bn)


if __name__ == "__main__":
    main()
