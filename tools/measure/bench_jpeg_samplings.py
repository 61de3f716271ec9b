"""Time the device JPEG decoder per sampling (4:2:0, 4:2:2, 4:4:4, greyscale) on panoramas, on one MI355X:

  * the rounds of pass B per chunk of the lane-parallel entropy stage -- counted by the HOST build of the same header
    (tests/host/jpeg_sampling_host.cpp, compiled here with g++ -O2; no GPU needed: `--rounds-only`), on the first panorama's scan;
  * the entropy stage and the inverse stage of BevRasteriser.jpeg_decode(entropy="lanes", sampling=) alone, by HIP events between the
    stages (`stages=`), on all panoramas in one call;
  * ingest.PanoStore.load(decode="device", samplings=jpeg.SAMPLINGS) end to end against the same call with the default keyword,
    by the host clock around a call that ends in a synchronise, the two calls alternating.  The default keyword sends a 4:2:2 / 4:4:4 / greyscale file to Pillow --
    what a checkout from before the keyword does with it -- so that IS the baseline; for 4:2:0, which the default already decodes on
    the device, the baseline is decode="host".  The two stores are compared after every pair.

Workload: --panos N (default 32) panoramas of 2048 x 1024 (synthetic.make_pano doubled, the ingest tests' content) written with Pillow at
--quality (default 90) in the sampling; the files come from the page cache.  Two warm-up calls, then --reps (default 7) timed ones:
medians (min .. max).

    python tools/measure/bench_jpeg_samplings.py [--panos 32] [--quality 90] [--reps 7] [--out FILE]
"""

from __future__ import annotations

import argparse
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from salve_amd import _lib, jpeg, synthetic  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

PILLOW_SUBSAMPLING = {"4:2:0": 2, "4:2:2": 1, "4:4:4": 0}
SEGMENT = np.dtype([("offset", "<i8"), ("bytes", "<i4"), ("image", "<i4"), ("first_mcu", "<i4"), ("mcu_count", "<i4")])


def _stat(ms):
    return f"{statistics.median(ms):8.2f} ({min(ms):.2f} .. {max(ms):.2f})"


def write_panos(root: Path, sampling: str, n: int, quality: int):
    from PIL import Image

    (root / "zind" / "0003" / "panos").mkdir(parents=True)
    fpaths = {}
    for i in range(n):
        rgb, depth = synthetic.make_pano(i)
        rgb = np.repeat(np.repeat(rgb, 2, axis=0), 2, axis=1)
        fp = root / "zind" / "0003" / "panos" / f"floor_01_partial_room_{i:02d}_pano_{i}.jpg"
        if sampling == "grey":
            Image.fromarray(rgb[..., 1]).save(str(fp), format="JPEG", quality=quality)
        else:
            Image.fromarray(rgb).save(str(fp), format="JPEG", quality=quality, subsampling=PILLOW_SUBSAMPLING[sampling])
        image_io.write_depth_png(str(root / "depth" / "0003" / f"{fp.stem}.depth.png"), depth)
        fpaths[i] = str(fp)
    return fpaths


def rounds_of(exe: Path, work: Path, data: bytes, p: jpeg.ParsedFile):
    """(rounds of pass B summed over the chunks, chunks) of one file's scan, from the host build of jpeg_entropy_lanes.h."""
    mcus = int(np.prod(jpeg.mcu_grid(p.h, p.w, p.sampling)))
    with open(work / "in.bin", "wb") as f:
        f.write(np.int32(1).tobytes() + np.int32(_lib.JPEG_SAMPLINGS[p.sampling]).tobytes() + np.ascontiguousarray(p.huffman, dtype=np.uint8).tobytes())
        f.write(np.array([mcus, len(data), len(p.segments)], dtype=np.int32).tobytes())
        f.write(np.array([(o, nb, 0, m0, mc) for o, nb, m0, mc in p.segments], dtype=SEGMENT).tobytes() + data)
    subprocess.run([str(exe), str(work / "in.bin"), str(work / "out.bin")], check=True)
    status, serial, rounds, same = (int(v) for v in np.frombuffer((work / "out.bin").read_bytes(), dtype=np.uint32, count=4))
    assert status == 0 and serial == 0 and same == 1
    text = (ROOT / "salve_amd" / "csrc" / "jpeg_entropy_lanes.h").read_text()
    import re

    chunk = int(re.search(r"#define JE_SUBSEQ (\d+)", text).group(1)) * int(re.search(r"#define JL_LANES (\d+)", text).group(1))
    return rounds, sum(-(-nb // chunk) for _, nb, _, _ in p.segments)


def bench(a, say) -> None:
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        exe = tmp / "jpeg_sampling_host"
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(ROOT / "tests" / "host" / "jpeg_sampling_host.cpp")], check=True)
        if not a.rounds_only:
            import torch

            from salve_amd import ingest
            from salve_amd.rasteriser import BevRasteriser

            dev = torch.device("cuda:0")
            ras = BevRasteriser(dev)
            say(f"device: {torch.cuda.get_device_name(0)}; subsequence {ras.lib.salve_bev_jpeg_subseq_bytes()} bytes; {a.panos} panoramas of 2048 x 1024, quality {a.quality}; "
                f"2 warm-up calls, {a.reps} timed: median (min .. max), ms")
        for sampling in jpeg.SAMPLINGS:
            root = tmp / sampling.replace(":", "")
            fpaths = write_panos(root, sampling, a.panos, a.quality)
            files = [Path(fpaths[i]).read_bytes() for i in range(a.panos)]
            parsed = [jpeg.parse_file(f, restart=True, samplings=jpeg.SAMPLINGS) for f in files]
            p = parsed[0]
            assert len({q.header_key for q in parsed}) == 1 and (p.h, p.w, p.sampling) == (1024, 2048, sampling)
            nb = np.array([q.scan_bytes for q in parsed])
            rounds, chunks = rounds_of(exe, tmp, files[0], p)
            say(f"\n{sampling}: {nb.mean() / 1024:.0f} KB of scan per panorama ({nb.min() / 1024:.0f} .. {nb.max() / 1024:.0f})")
            say(f"    pass B on the first panorama's scan: {rounds} rounds in {chunks} chunks, {rounds / chunks:.1f} per chunk")
            if a.rounds_only:
                continue
            off = np.cumsum(np.r_[0, nb])
            blob = b"".join(f[q.scan_offset:q.scan_offset + q.scan_bytes] for f, q in zip(files, parsed)) + bytes(jpeg.SCAN_PADDING)
            scans = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
            out = torch.empty((a.panos, p.h, p.w), dtype=torch.int32, device=dev)
            fn = lambda **more: ras.jpeg_decode(scans, off[:-1], nb, p.h, p.w, p.qtab, p.huffman, out=out, entropy="lanes", sampling=sampling, **more)
            for _ in range(2):
                _, st = fn()
            torch.cuda.synchronize()
            assert not bool(st.any())
            want = torch.from_numpy(np.stack([ingest._read_rgb3(fpaths[i]) for i in (0, a.panos - 1)])).to(dev)
            assert torch.equal(ras.export_u8(out[[0, a.panos - 1]]), want), "the device's pixels differ from Pillow's"
            ent, inv = [], []
            for _ in range(a.reps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                fn(stages=_lib.JPEG_STAGE_ENTROPY)
                ev[1].record()
                fn(stages=_lib.JPEG_STAGE_INVERSE)
                ev[2].record()
                ev[2].synchronize()
                ent.append(ev[0].elapsed_time(ev[1]))
                inv.append(ev[1].elapsed_time(ev[2]))
            say(f"    entropy stage (lanes, with its two clears) {_stat(ent)}    inverse stage {_stat(inv)}")
            del out, scans
            routes = {"baseline": dict(decode="host") if sampling == "4:2:0" else dict(decode="device"),
                      "device": dict(decode="device", samplings=jpeg.SAMPLINGS)}
            stores, times = {}, {tag: [] for tag in routes}
            for r in range(a.reps + 2):          # the two routes ALTERNATE, so that what else the host is doing meets both alike
                for tag, kw in routes.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    stores[tag] = ingest.PanoStore(dev).load(fpaths, str(root / "depth"), "0003", list(range(a.panos)), **kw)
                    torch.cuda.synchronize()
                    if r >= 2:
                        times[tag].append((time.perf_counter() - t) * 1e3)
            same = torch.equal(stores["baseline"].rgb, stores["device"].rgb) and torch.equal(stores["baseline"].depth, stores["device"].depth)
            base = 'decode="host"' if sampling == "4:2:0" else 'decode="device", default samplings'
            say(f"    PanoStore.load, {base}: {_stat(times['baseline'])}  [{stores['baseline'].host_decoded if sampling != '4:2:0' else a.panos} files by Pillow]")
            say(f"    PanoStore.load, decode=\"device\", samplings=jpeg.SAMPLINGS: {_stat(times['device'])}  [{stores['device'].host_decoded} files by Pillow]")
            say(f"    ratio of the medians {statistics.median(times['baseline']) / statistics.median(times['device']):.2f} x; the two stores: {'bit-identical' if same else 'DIFFERENT'}")
            del stores


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--panos", type=int, default=32)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds-only", action="store_true", help="the rounds of pass B alone: the host build, no GPU")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("\n".join(lines) + "\n")

    bench(a, say)
