"""Training the verifier: the reference's training helpers and loop (salve/train_utils.py, scripts/train.py) on the HIP fp32
training convolutions.

Same names as the reference: get_model, get_optimizer, poly_learning_rate, cross_entropy_forward, get_train_transform,
get_dataloader, run_epoch, plus `train` (scripts/train.py:41-119's main) and `train_rendered`, the same loop fed by batches
rendered on the GPU (salve_amd.train_render) instead of the rendered dataset on disk.  The model is
salve_amd.models.trainable.TrainableEarlyFusionCEResnet (its checkpoints load into the inference EarlyFusionCEResnet with
strict=True).  salve_amd.train_utils stays inference-only and keeps refusing the train split: training is reached through this
module (and `python -m salve_amd.train`) only.

Differences from the reference, all deliberate: one GPU per process (`dataparallel` is accepted and ignored, the state dict carries
no `module.` prefix; several GPUs train data-parallel with one process each: `dist=`, salve_amd.dist_train, `--gpus N`), num_workers = 0 (the transforms launch GPU kernels), photometric augmentation (False in every released config; opt-in: photometric="device")
and crop-with-padding are refused, the shuffle order comes from a seeded torch.Generator.
"""

from __future__ import annotations

import json
import logging
import random
import time
from collections import defaultdict
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from salve_amd.dist_train import DataParallel, bn_statistics
from salve_amd.evaluate import ClassAccuracyMeter, DeviceClassMeter
from salve_amd.models.trainable import TRAIN_HEADS, TRAIN_NORMS, TRAIN_PRECISIONS, TrainableEarlyFusionCEResnet
from salve_amd.optim import OPTIMS, HipAdam
from salve_amd.training_config import TrainingConfig

CRIT_ACC_STAT = "val_mAcc"   # scripts/train.py:85: the checkpoint-selection criterion


def _check_precision(precision: str) -> None:
    if precision not in TRAIN_PRECISIONS:
        raise ValueError(f"training precision must be one of {TRAIN_PRECISIONS}, got {precision!r}")


def _check_norm(norm: str) -> None:
    if norm not in TRAIN_NORMS:
        raise ValueError(f"training norm must be one of {TRAIN_NORMS}, got {norm!r}")


def _check_sync_bn(sync_bn: bool, norm: str) -> None:
    if sync_bn and norm != "hip":
        raise ValueError(f'sync_bn=True (--sync-bn) synchronises the statistics of the HIP BatchNorm: it needs norm="hip" (--norm hip), got {norm!r}')


def _check_optim(optim: str) -> None:
    if optim not in OPTIMS:
        raise ValueError(f"training optimiser must be one of {OPTIMS}, got {optim!r}")


def _check_head(head: str) -> None:
    if head not in TRAIN_HEADS:
        raise ValueError(f"training head must be one of {TRAIN_HEADS}, got {head!r}")


def get_model(args: TrainingConfig, precision: str = "fp32", norm: str = "torch", head: str = "torch") -> nn.Module:
    """TrainableEarlyFusionCEResnet on the GPU (salve/train_utils.py:205-217).  `args.dataparallel` is accepted and ignored: the
    model is never wrapped; data-parallel training is one process per GPU around the same model (`train(..., dist=)`).
    precision: "fp32" (the reference's) or "bf16" (opt-in mixed precision: TrainableEarlyFusionCEResnet.set_train_precision).
    norm: "torch" (nn.BatchNorm2d) or "hip" (opt-in fused HIP BatchNorm: TrainableEarlyFusionCEResnet.set_train_norm).
    head: "torch" (avgpool, fc, softmax, cross_entropy) or "hip" (opt-in fused HIP classifier head with the loss and the accuracy
    counts kept on the device: TrainableEarlyFusionCEResnet.set_train_head)."""
    _check_precision(precision)
    _check_norm(norm)
    _check_head(head)
    if not torch.cuda.is_available():
        raise RuntimeError("salve_amd.training needs the HIP device (no CPU fallback)")
    model = TrainableEarlyFusionCEResnet(args.num_layers, args.pretrained, args.num_ce_classes, args)
    return model.set_train_precision(precision).set_train_norm(norm).set_train_head(head).cuda()


def get_optimizer(args: TrainingConfig, model: nn.Module, optim: str = "torch") -> torch.optim.Optimizer:
    """Adam(lr=base_lr, weight_decay) -- the only algorithm the reference knows (salve/train_utils.py:173-180).
    optim: "torch" (torch.optim.Adam) or "hip" (opt-in: salve_amd.optim.HipAdam, the same update in one HIP launch, the same
    state and state dict; for a model that trains in bf16 it also keeps the convolution weights' bf16 copies current)."""
    _check_optim(optim)
    if args.optimizer_algo == "adam":
        if optim == "hip":
            return HipAdam(model.parameters(), lr=args.base_lr, weight_decay=args.weight_decay,
                           bf16_shadow=getattr(model, "train_precision", "fp32") == "bf16")
        return torch.optim.Adam(model.parameters(), lr=args.base_lr, weight_decay=args.weight_decay)
    raise RuntimeError("Unknown optimizer")


def poly_learning_rate(base_lr: float, curr_iter: int, max_iter: int, power: float = 0.9) -> float:
    """poly learning rate policy (salve/train_utils.py:57-60)."""
    return base_lr * (1 - float(curr_iter) / max_iter) ** power


def cross_entropy_forward(model: nn.Module, split: str, x1: Tensor, x2: Tensor, x3: Optional[Tensor], x4: Optional[Tensor],
                          x5: Optional[Tensor], x6: Optional[Tensor], is_match: Tensor, meters: Optional[DeviceClassMeter] = None,
                          accumulate_loss: bool = False) -> Tuple[Tensor, Tensor]:
    """(softmax probabilities, cross-entropy loss) as salve/train_utils.py:18-41: with gradients for split == "train", under
    torch.no_grad() otherwise.  A model whose head is "hip" goes through its `forward_loss` (meters, accumulate_loss: see there)."""
    if getattr(model, "train_head", "torch") == "hip":
        with torch.set_grad_enabled(split == "train" and torch.is_grad_enabled()):
            return model.forward_loss(x1, x2, x3, x4, x5, x6, is_match, meters=meters, accumulate_loss=accumulate_loss)
    if split == "train":
        logits = model(x1, x2, x3, x4, x5, x6)
    else:
        with torch.no_grad():
            logits = model(x1, x2, x3, x4, x5, x6)
    probs = torch.nn.functional.softmax(logits.detach().clone(), dim=1)
    loss = torch.nn.functional.cross_entropy(logits, is_match.reshape(-1))   # ([B, 1] or [B]; a one-row batch -- a rank's slice of a short one -- stays [1])
    return probs, loss


def cross_entropy_forward_packed(model: nn.Module, split: str, x_packed: Tensor, is_match: Tensor, meters: Optional[DeviceClassMeter] = None,
                                 accumulate_loss: bool = False) -> Tuple[Tensor, Tensor]:
    """`cross_entropy_forward` for the packed input of salve_amd.train_render ([B, H, W, Cp], `model.forward_packed`)."""
    if getattr(model, "train_head", "torch") == "hip":
        with torch.set_grad_enabled(split == "train" and torch.is_grad_enabled()):
            return model.forward_packed_loss(x_packed, is_match, meters=meters, accumulate_loss=accumulate_loss)
    if split == "train":
        logits = model.forward_packed(x_packed)
    else:
        with torch.no_grad():
            logits = model.forward_packed(x_packed)
    probs = torch.nn.functional.softmax(logits.detach().clone(), dim=1)
    loss = torch.nn.functional.cross_entropy(logits, is_match.reshape(-1))   # ([B, 1] or [B]; a one-row batch -- a rank's slice of a short one -- stays [1])
    return probs, loss


def _jitter(args: TrainingConfig, photometric: Optional[str]) -> Optional[str]:
    """What a feed is built with: `photometric` only permits, the config's field decides."""
    return photometric if args.apply_photometric_augmentation else None


def get_train_transform(args: TrainingConfig, photometric: Optional[str] = None):
    """Resize -> [PhotometricShift ->] random Crop -> random horizontal flip -> random vertical flip -> ToTensor -> Normalize for
    2 / 4 / 6 images (salve/train_utils.py:63-124), on the GPU (transforms.TrainTransform).  photometric: None (default) refuses a config
    with apply_photometric_augmentation=True, as before the augmentation existed; "device" accepts it -- ColorJitter on the device, every
    image with draws of its own.  With the field False the keyword changes nothing."""
    from salve_amd.train_feed import JITTER_TYPES, check_photometric
    from salve_amd.transforms import TrainTransform

    check_photometric(photometric)
    if len(args.modalities) not in (1, 2, 3):
        raise RuntimeError(f"Unsupported modalities. {str(args.modalities)}")
    if args.apply_photometric_augmentation and photometric is None:
        raise RuntimeError("apply_photometric_augmentation=True (PhotometricShift) is opt-in: pass photometric=\"device\" (--photometric device) "
                           "to run the photometric augmentation on the device; every released config has False")
    if args.train_h > args.resize_h or args.train_w > args.resize_w:
        raise RuntimeError("crop larger than the resized image: the reference pads with the mean there, which is not implemented")
    return TrainTransform((args.resize_h, args.resize_w), (args.train_h, args.train_w),
                          jitter_types=JITTER_TYPES if _jitter(args, photometric) else None)


DECODES = ("host", "device")


def _check_decode(decode: str) -> None:
    if decode not in DECODES:
        raise ValueError(f"decode must be one of {DECODES}, got {decode!r}")


def get_tile_file_source(args: TrainingConfig, split: str, seed: int = 0, precision: str = "fp32", entropy: str = "image",
                         read_ahead: bool = False, photometric: Optional[str] = None, rank: int = 0, world: int = 1):
    """`get_dataloader`'s examples in its order as a train_files.TileFileSource: whole batches of the data set's JPEG tiles decoded
    on the device, `(x_packed, is_match)` for `run_epoch`.  Grouping and ordering are ZindData's.  entropy, read_ahead: TileFileSource's.
    photometric: `get_train_transform`'s keyword (the train split jitters iff the config's field is True).
    rank, world: TileFileSource's (data-parallel training: this rank's rows of every batch)."""
    from salve_amd.dataset.zind_data import ZindData
    from salve_amd.train_files import TileFileSource

    get_train_transform(args, photometric)   # (the refusals of the host path: photometric augmentation without the keyword, crop-with-padding)
    data = ZindData(split=split, transform=None, args=args)
    return TileFileSource(torch.device("cuda", torch.cuda.current_device()), data.data_list, batch_size=args.batch_size, precision=precision,
                          split=split, seed=seed, resize_hw=(args.resize_h, args.resize_w), crop_hw=(args.train_h, args.train_w), entropy=entropy,
                          read_ahead=read_ahead, photometric=_jitter(args, photometric), rank=rank, world=world)


def get_dataloader(args: TrainingConfig, split: str, seed: int = 0, photometric: Optional[str] = None) -> torch.utils.data.DataLoader:
    """salve/train_utils.py:183-203.  train: the train transform, shuffled (a torch.Generator seeded with `seed`), last partial
    batch dropped; val / test: the centre-crop transform, in order, nothing dropped.  num_workers = 0.  photometric:
    `get_train_transform`'s keyword; val / test never jitter."""
    from salve_amd import train_utils
    from salve_amd.dataset.zind_data import ZindData

    if split == "train":
        data = ZindData(split=split, transform=get_train_transform(args, photometric), args=args)
        gen = torch.Generator()
        gen.manual_seed(seed)
        return torch.utils.data.DataLoader(data, batch_size=args.batch_size, shuffle=True, generator=gen, num_workers=0, drop_last=True)
    data = ZindData(split=split, transform=train_utils.get_img_transform_list(args, split), args=args)
    return torch.utils.data.DataLoader(data, batch_size=args.batch_size, shuffle=False, num_workers=0, drop_last=False)


def _unpack(args: TrainingConfig, example):
    m = set(args.modalities)
    if len(m) == 1:
        x1, x2, is_match, fp0, fp1 = example
        return (x1, x2, None, None, None, None), is_match
    if m == {"ceiling_rgb_texture", "floor_rgb_texture"}:
        x1, x2, x3, x4, is_match, fp0, fp1 = example
        return (x1, x2, x3, x4, None, None), is_match
    x1, x2, x3, x4, x5, x6, is_match, fp0, fp1 = example
    return (x1, x2, x3, x4, x5, x6), is_match


def _log(dist: Optional[DataParallel]) -> bool:
    """Whether this process logs and writes files: rank 0 does."""
    return dist is None or dist.is_main


def _local(dist: Optional[DataParallel]) -> str:
    """What a per-iteration log line says of its loss when several ranks train: it is this rank's rows' alone."""
    return f" (rank 0's rows of {dist.world} ranks)" if dist is not None and dist.world > 1 else ""


def run_epoch(args: TrainingConfig, epoch: int, model: nn.Module, data_loader, optimizer: torch.optim.Optimizer, split: str,
              dist: Optional[DataParallel] = None) -> Dict[str, float]:
    """One pass over a split (scripts/train.py:169-278): train mode + Adam steps + the poly schedule for "train", eval mode
    otherwise.  Returns {"avg_loss", "mAcc"}; as in the reference, avg_loss counts training batches only (0 for val).
    `data_loader`: a DataLoader over ZindData, or a train_render.RenderedTrainSource (2-tuples, through `model.forward_packed`).
    A model whose head is "hip" runs `_run_epoch_device`: the same pass without a wait for the device between batches.
    dist (data-parallel training): the loader yields this rank's rows; the ranks' gradients are averaged between backward and step
    (DataParallel.all_reduce_gradients), counts and loss sums are summed over the ranks once, at the end of the pass, so every rank
    returns the same dict; only rank 0 logs, and the loss it logs per iteration is its own rows'."""
    if getattr(model, "train_head", "torch") == "hip":
        return _run_epoch_device(args, epoch, model, data_loader, optimizer, split, dist)
    model.train() if split == "train" else model.eval()
    loss_sum, loss_n = 0.0, 0
    meter = ClassAccuracyMeter(args.num_ce_classes)
    dev = next(model.parameters()).device
    max_iter = args.num_epochs * len(data_loader)
    t0 = time.time()
    for it, example in enumerate(data_loader):
        if len(example) == 2:   # (x_packed, is_match) of a train_render.RenderedTrainSource: on the device, in the stem's layout
            xs, gt = (example[0],), example[1]
            probs, loss = cross_entropy_forward_packed(model, split, xs[0], gt)
        else:
            xs, is_match = _unpack(args, example)
            xs = tuple(None if x is None else x.to(dev, non_blocking=True) for x in xs)
            gt = is_match.to(dev, non_blocking=True)
            probs, loss = cross_entropy_forward(model, split, *xs, gt)
        meter.update(torch.argmax(probs, dim=1).cpu().numpy(), gt.squeeze().cpu().numpy())
        current_iter = epoch * len(data_loader) + it + 1
        if split == "train":
            optimizer.zero_grad()
            loss.backward()
            if dist is not None:
                dist.all_reduce_gradients(model.parameters())
            optimizer.step()
            if args.lr_annealing_strategy == "poly":   # decayed after the step, as the reference does
                lr = poly_learning_rate(args.base_lr, current_iter, max_iter, power=args.poly_lr_power)
                for group in optimizer.param_groups:
                    group["lr"] = lr
            n = xs[0].shape[0]
            loss_sum += float(loss.item()) * n
            loss_n += n
            if it % max(1, args.print_every) == 0 and _log(dist):
                logging.info(f"\t{split} iter [{it + 1}/{len(data_loader)}] loss {loss.item():.4f}{_local(dist)} ({time.time() - t0:.1f} s)")
    if dist is not None:
        loss_sum, loss_n = dist.reduce_meter(meter, loss=(loss_sum, loss_n))
    accs, mAcc = meter.get_metrics()
    if _log(dist):
        logging.info(f"{split} result at epoch [{epoch + 1}/{args.num_epochs}]: mAcc {mAcc:.4f}, class accuracies {accs.tolist()}")
    return {"avg_loss": loss_sum / loss_n if loss_n else 0.0, "mAcc": float(mAcc)}


def _run_epoch_device(args: TrainingConfig, epoch: int, model: nn.Module, data_loader, optimizer: torch.optim.Optimizer, split: str,
                      dist: Optional[DataParallel] = None) -> Dict[str, float]:
    """`run_epoch` for a model with the HIP head: the loss sum and the per-class counts live in a DeviceClassMeter that the head's
    forward updates, so no batch copies anything to the host -- the host enqueues batch after batch and reads the meter once at the
    end of the pass.  Only the iterations that log (`it % print_every == 0`, training) read their loss.  Same schedule, same
    returned dict.  dist: `run_epoch`'s; the device record is summed over the ranks before its one read."""
    model.train() if split == "train" else model.eval()
    dev = next(model.parameters()).device
    meter = DeviceClassMeter(args.num_ce_classes, dev)
    max_iter = args.num_epochs * len(data_loader)
    t0 = time.time()
    train = split == "train"
    for it, example in enumerate(data_loader):
        if len(example) == 2:
            probs, loss = cross_entropy_forward_packed(model, split, example[0], example[1], meters=meter, accumulate_loss=train)
        else:
            xs, is_match = _unpack(args, example)
            xs = tuple(None if x is None else x.to(dev, non_blocking=True) for x in xs)
            probs, loss = cross_entropy_forward(model, split, *xs, is_match.to(dev, non_blocking=True), meters=meter, accumulate_loss=train)
        current_iter = epoch * len(data_loader) + it + 1
        if train:
            optimizer.zero_grad()
            loss.backward()
            if dist is not None:
                dist.all_reduce_gradients(model.parameters())
            optimizer.step()
            if args.lr_annealing_strategy == "poly":   # decayed after the step, as the reference does
                lr = poly_learning_rate(args.base_lr, current_iter, max_iter, power=args.poly_lr_power)
                for group in optimizer.param_groups:
                    group["lr"] = lr
            if it % max(1, args.print_every) == 0 and _log(dist):
                logging.info(f"\t{split} iter [{it + 1}/{len(data_loader)}] loss {loss.item():.4f}{_local(dist)} ({time.time() - t0:.1f} s)")
    if dist is not None:
        dist.reduce_meter(meter)
    accs, mAcc, avg_loss = meter.read()
    if _log(dist):
        logging.info(f"{split} result at epoch [{epoch + 1}/{args.num_epochs}]: mAcc {mAcc:.4f}, class accuracies {accs.tolist()}")
    return {"avg_loss": avg_loss, "mAcc": float(mAcc)}


def train(args: TrainingConfig, results_dir: str, seed: int = 0, init_ckpt: Optional[str] = None, precision: str = "fp32",
          norm: str = "torch", optim: str = "torch", head: str = "torch", decode: str = "host", entropy: str = "image",
          read_ahead: bool = False, photometric: Optional[str] = None, dist: Optional[DataParallel] = None,
          sync_bn: bool = False) -> Dict[str, list]:
    """scripts/train.py:41-119: seeds, loaders, model, optimiser, then per epoch a train pass and a val pass under no_grad.  On
    epoch 0 and on every improvement of val_mAcc, `{results_dir}/train_ckpt.pth` is written with the reference's keys; the
    results JSON (`results-{cfg_stem}.json`, train_* / val_* series) is rewritten every epoch.  init_ckpt: fine-tune from a
    checkpoint's state dict (strict).  precision: "fp32" (default) or "bf16" -- the checkpoint is fp32 either way (fp32 master
    weights), with the same keys.  norm: "torch" (default) or "hip", the fused HIP BatchNorm -- same parameters, buffers and
    checkpoint.  optim: "torch" (default) or "hip", HipAdam -- the checkpoint's "optimizer" entry keeps torch.optim.Adam's format.
    head: "torch" (default) or "hip", the fused HIP classifier head with loss and accuracy on the device -- same results JSON.
    decode: "host" (default: Pillow decodes every tile in the DataLoader) or "device": the same examples in the same order with the
    same draws, whole batches of JPEG tiles decoded on the device (train_files.TileFileSource) -- the same batches, bit for bit.
    entropy (decode="device" only): "image" (default) or "lanes", the lane-parallel entropy stage, which also keeps files with restart
    intervals on the device -- the same batches again.
    read_ahead (decode="device" only; default False): the next batches' files are read, and the next batch decoded on a side stream,
    while the current batch trains (TileFileSource(read_ahead=True)) -- the same batches once more.
    photometric: None (default) or "device" -- a config with apply_photometric_augmentation=True trains only with "device": the
    reference's PhotometricShift on the device in every train batch of either decode; val batches never jitter.
    dist: None (default), or a dist_train.DataParallel: this process is one of `dist.world` ranks, each of which trains its rows of
    every batch; needs decode="device" in a world larger than one -- the host DataLoader draws inside its worker
    processes and is not sharded.  Rank 0 logs and writes the checkpoint and the results JSON; every rank returns the same dict.
    sync_bn (default False; needs norm="hip"): every train-mode BatchNorm normalises over the rows of all `dist.world` ranks
    (SyncBatchNormHipFunction), and every rank keeps the same running statistics; without a `dist` that runs
    collectives (None, or a world of one that is not forced) it changes nothing."""
    _check_precision(precision)
    _check_norm(norm)
    _check_sync_bn(sync_bn, norm)
    _check_optim(optim)
    _check_head(head)
    _check_decode(decode)
    if entropy != "image" and decode != "device":
        raise ValueError(f'entropy={entropy!r} selects the device decoder\'s entropy stage: it needs decode="device"')
    if read_ahead and decode != "device":
        raise ValueError('read_ahead=True reads the device decoder\'s next batch ahead: it needs decode="device"')
    rank, world = (dist.rank, dist.world) if dist is not None else (0, 1)
    if world > 1 and decode != "device":
        raise ValueError(f'data-parallel training over {world} ranks needs decode="device" (--decode device): the host DataLoader feed '
                         "(decode=\"host\") takes its draws inside worker processes and is not sharded")
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    if decode == "device":
        with get_tile_file_source(args, "train", seed, precision, entropy, read_ahead, photometric, rank, world) as train_source, \
                get_tile_file_source(args, "val", seed, precision, entropy, read_ahead, photometric, rank, world) as val_source:
            return _fit(args, train_source, val_source, results_dir, init_ckpt, precision, norm, optim, head, dist, sync_bn)   # (leaving ends their reader threads)
    return _fit(args, get_dataloader(args, "train", seed=seed, photometric=photometric), get_dataloader(args, "val"), results_dir, init_ckpt,
                precision, norm, optim, head, dist, sync_bn)


def train_rendered(args: TrainingConfig, train_source, val_source, results_dir: str, seed: int = 0, init_ckpt: Optional[str] = None,
                   precision: str = "fp32", norm: str = "torch", optim: str = "torch", head: str = "torch",
                   jpeg_quality: Optional[int] = None, photometric: Optional[str] = None, dist: Optional[DataParallel] = None,
                   sync_bn: bool = False) -> Dict[str, list]:
    """`train` fed by two train_render.RenderedTrainSource objects (split "train", built with the same `seed` and `precision`, and
    split "val") instead of the rendered dataset on disk: the same epoch loop, checkpoint and results JSON.  jpeg_quality: the
    sources' own argument (the reference's JPEG round trip of every rendered image, on the device); the two sources must agree, and
    an integer given here must be what they were built with.  photometric: `train`'s keyword; the train source must have been built
    with what the config and the keyword amount to (RenderedTrainSource(photometric=)).  dist: `train`'s; both sources must have been
    built with its rank and world (RenderedTrainSource(rank=, world=)).  sync_bn: `train`'s."""
    _check_precision(precision)
    _check_norm(norm)
    _check_sync_bn(sync_bn, norm)
    _check_optim(optim)
    _check_head(head)
    get_train_transform(args, photometric)   # (the refusals of the on-disk path: photometric augmentation without the keyword, crop-with-padding)
    if getattr(train_source, "photometric", None) != _jitter(args, photometric):
        raise RuntimeError(f"the train source was built with photometric={getattr(train_source, 'photometric', None)!r}; the config's "
                           f"apply_photometric_augmentation={args.apply_photometric_augmentation} and photometric={photometric!r} ask for "
                           f"{_jitter(args, photometric)!r}")
    rank, world = (dist.rank, dist.world) if dist is not None else (0, 1)
    for src in (train_source, val_source):
        if (getattr(src, "rank", 0), getattr(src, "world", 1)) != (rank, world):
            raise RuntimeError(f"a batch source was built for rank {getattr(src, 'rank', 0)} of {getattr(src, 'world', 1)}, this process is "
                               f"rank {rank} of {world}")
    want = torch.bfloat16 if precision == "bf16" else torch.float32
    for src in (train_source, val_source):
        if src.dtype != want:
            raise RuntimeError(f"the batch source yields {src.dtype}, training precision {precision} takes {want}")
    built = (getattr(train_source, "jpeg_quality", None), getattr(val_source, "jpeg_quality", None))
    if built[0] != built[1] or (jpeg_quality is not None and built[0] != int(jpeg_quality)):
        raise RuntimeError(f"the batch sources were built with jpeg_quality {built[0]} (train) and {built[1]} (val), "
                           f"train_rendered was asked for {jpeg_quality}: build both with the same value")
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    return _fit(args, train_source, val_source, results_dir, init_ckpt, precision, norm, optim, head, dist, sync_bn)


def _fit(args: TrainingConfig, train_loader, val_loader, results_dir: str, init_ckpt: Optional[str], precision: str, norm: str,
         optim: str = "torch", head: str = "torch", dist: Optional[DataParallel] = None, sync_bn: bool = False) -> Dict[str, list]:
    """The epoch loop of `train` / `train_rendered` (scripts/train.py:60-119) on two batch sources.  dist: every rank starts from
    rank 0's parameters (one broadcast), validates with rank 0's BatchNorm statistics (one broadcast in front of every val pass: the
    reference's DataParallel keeps replica 0's), and rank 0 alone writes the checkpoint and the results JSON.  sync_bn: the train
    batches' BatchNorm statistics are taken over all ranks' rows (the train batch is `args.batch_size` rows, split in equal
    blocks); every rank then holds rank 0's running statistics already, and the broadcast copies what is there."""
    if len(train_loader) == 0:
        raise RuntimeError(f"the train split has fewer than batch_size={args.batch_size} examples")
    _check_sync_bn(sync_bn, norm)
    model = get_model(args, precision, norm, head)
    if sync_bn and dist is not None:
        model.set_sync_norm(dist, batch_size=args.batch_size)
    if init_ckpt:
        from salve_amd import train_utils

        train_utils.load_model_checkpoint(init_ckpt, model, args)
    if dist is not None:
        dist.broadcast(list(model.parameters()))
    optimizer = get_optimizer(args, model, optim)
    out = Path(results_dir)
    if _log(dist):
        out.mkdir(parents=True, exist_ok=True)
    results: Dict[str, list] = defaultdict(list)
    for epoch in range(args.num_epochs):
        if _log(dist):
            logging.info(f"On epoch {epoch}")
        for k, v in run_epoch(args, epoch, model, train_loader, optimizer, "train", dist).items():
            results[f"train_{k}"].append(v)
        if dist is not None:
            dist.broadcast(bn_statistics(model))
        with torch.no_grad():
            for k, v in run_epoch(args, epoch, model, val_loader, optimizer, "val", dist).items():
                results[f"val_{k}"].append(v)
        if not _log(dist):
            continue
        crit = results[CRIT_ACC_STAT]
        if epoch == 0 or crit[-1] > max(crit[:-1]):
            torch.save({
                "epoch": epoch,
                "state_dict": model.state_dict(),
                "optimizer": optimizer.state_dict(),
                "max_epochs": args.num_epochs,
                f"curr_{CRIT_ACC_STAT}": crit[-1],
                f"best_so_far_{CRIT_ACC_STAT}": max(crit),
            }, out / "train_ckpt.pth")
        with open(out / f"results-{args.cfg_stem}.json", "w") as f:
            json.dump(dict(results), f, indent=4)
    return dict(results)
