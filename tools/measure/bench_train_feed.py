"""Time the rendered training feed (salve_amd.train_render) beside the training step it feeds, on one MI355X:

  * the source alone, per batch: host clock around one batch + synchronise, and HIP events around its scatter / densify / tile launches;
    the tile launch also as a rate of algorithmic bytes (the batch tensor written + the BEV images of the batch read once);
  * the training step (forward + backward + Adam) three ways, alternating step by step in one process: resident NCHW tensors through
    `forward` (what tools/measure/bench_train.py times), the resident packed tensor through `forward_packed`, and a batch rendered by
    the source through `forward_packed` (feed included);
  * --disk N: end-to-end samples/s of `training.run_epoch` over N batches from the source and from the on-disk path -- the same
    examples written once as JPEGs into a temporary ZindData tree (outside the timed region) and fed by `training.get_dataloader`.

    python tools/measure/bench_train_feed.py [--configs 152:2,50:1] [--batch 256] [--modes bf16:hip,fp32:torch] [--steps 5] [--warmup 2]
                                             [--panos 64] [--disk 0] [--identity {kept,batch}] [--resident-panos N [--prefetch]] [--layout]

--identity batch and / or --resident-panos N switch to the comparison of the feed's modes instead: rows (a) identity
"kept", everything resident (the default source: the yardstick), (b) identity "batch", everything resident, and with --resident-panos
(c) a pool of N slots in its second epoch (steady state) and (d) in its first (cold fill) -- source alone with the event split (upload and
index update beside scatter, densify, tiles), the host-to-device rate reached, the uploads per batch the planner makes (furthest next
use) beside what LRU would make on the same epochs, and the step fed by each row beside the step on a resident batch.  --panos P must
then be at least 4 x batch (so that a half-size pool misses); the P scenes are distinct (a few rooms, each turned by its own angle).
--prefetch adds row (e): the same pool with prefetch=True (the pool must hold 4 x batch).  A prefetched upload hides under
the step that FOLLOWS its submission, so row (e) is not part of the step-by-step alternation (there four other rows' steps would run before
its next batch is asked for, and its upload would land under them): it is timed over CONSECUTIVE steps of whole epochs, the way training
consumes it -- every step ends with `loss.item()` as training.run_epoch's does, the device is synchronised once, behind the epoch --
with three kinds of epoch alternating epoch by epoch in one process: the resident batch, row (c) (the same pool size without prefetch: the
yardstick) and row (e).  The first round (the pools' cold fill) is dropped.  Reported per kind: the median step behind an epoch's first, the
first step (made resident serially in both rows), the epoch's time per batch, and for (e) the host time its loop spent waiting for upload jobs.

--layout switches to the layout modality with synthetic layouts (salve_amd/synthetic_layouts.py): per batch the HIP
events of the pose / rasterise / tile launches, the source alone, and the fed step beside the resident step for ResNet-50 on layout
alone (6 channels) and ResNet-152 on ceiling + floor + layout (18 channels), bf16 + hip norm -- and, as the yardstick of posing on the
device, the SAME batch posed by the existing host path (`pack_layouts` of 2 x batch specs, its upload included).

Synthetic 1024 x 512 panoramas (as bench.py).  Medians; run the command twice for the spread.  Per-kernel times: a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/measure/bench_train_feed.py ...`.
"""

from __future__ import annotations

import argparse
import random
import shutil
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from salve_amd import synthetic, train_render, training  # noqa: E402
from salve_amd.models import trainable  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402

MODS = {1: ["floor_rgb_texture"], 2: ["ceiling_rgb_texture", "floor_rgb_texture"]}
COPY_TBS = 5.3   # the measured float4 copy rate (profiles/r06_copy_sweep.txt)


def med(v):
    return sorted(v)[len(v) // 2]


def config(layers: int, nm: int, batch: int, data_root: str = "") -> TrainingConfig:
    return TrainingConfig(lr_annealing_strategy="poly", base_lr=1e-4, weight_decay=1e-4, num_ce_classes=2, print_every=10 ** 9, poly_lr_power=0.9,
                          optimizer_algo="adam", num_layers=layers, pretrained=False, dataparallel=False, resize_h=234, resize_w=234, train_h=224,
                          train_w=224, apply_photometric_augmentation=False, modalities=tuple(MODS[nm]), cfg_stem="feed", num_epochs=1, workers=0,
                          batch_size=batch, data_root=data_root, layout_data_root="", model_save_dirpath="")


def step(model, opt, fwd, y):
    opt.zero_grad(set_to_none=True)
    F.cross_entropy(fwd(), y).backward()
    opt.step()


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def write_zind_tree(root: Path, src, n: int) -> None:
    """Examples 0 .. n-1 of `src` as the reference's rendered dataset: {root}/{label}/{building}/pair_{k}___..._{surface}_rgb_floor_01_..._pano_{id}.jpg
    (building 1208 is in the official train split).  The JPEGs are the source's own renders -- lossy, as the on-disk path's inputs are."""
    from salve_amd.rasteriser import SURFACES, pack_hypotheses
    from salve_amd.utils import image_io

    ex, S = src.examples, len(src.surfaces)
    surf = [SURFACES[s] for s in src.surfaces]
    ident = src.ras.export_u8(src.ref_bev).cpu().numpy()
    for lo in range(0, n, 64):
        m = min(64, n - lo)
        idx = np.arange(lo, lo + m)
        rows = pack_hypotheses(np.repeat(ex["i1"][idx], S), np.tile(surf, m), np.repeat(ex["R"][idx], S, axis=0), np.repeat(ex["t"][idx], S, axis=0), np.ones(m * S))
        bev, _ = src.ras.render(src.pano_rgb, src.pano_depth, src.ras.upload_hypotheses(rows), m * S)
        posed = src.ras.export_u8(bev).cpu().numpy()
        for k, j in enumerate(idx):
            label = "gt_alignment_approx" if ex["is_match"][j] else "incorrect_alignment"
            d = root / label / "1208"
            d.mkdir(parents=True, exist_ok=True)
            if S == 1:   # ZindData groups a pair's FOUR tiles, whichever modalities are read: the other surface's files exist, unread
                other = "ceiling" if src.surfaces[0] == "floor" else "floor"
                for pid in (2 * int(j), 2 * int(j) + 1):
                    image_io.write_jpeg(str(d / f"pair_{j}___door_0_0_rotated_{other}_rgb_floor_01_partial_room_01_pano_{pid}.jpg"), posed[k])
            for si, name in enumerate(src.surfaces):
                stem = f"pair_{j}___door_0_0_rotated_{name}_rgb_floor_01_partial_room_01_pano_"
                # (two distinct pano ids per pair; which tile the loader puts first does not matter to a timing)
                image_io.write_jpeg(str(d / f"{stem}{2 * int(j)}.jpg"), posed[k * S + si])
                image_io.write_jpeg(str(d / f"{stem}{2 * int(j) + 1}.jpg"), ident[int(ex["i2"][j]) * S + si])


def distinct_panos(P: int, base: int = 64):
    """P distinct 1024 x 512 scenes without P ray casts: `base` synthetic rooms, each also seen turned about the vertical axis (the
    panorama and its depth map rolled by the same number of columns -- another room as far as the renderer is concerned)."""
    rooms = synthetic.make_panos(min(P, base))
    rgb = np.empty((P,) + rooms[0][0].shape, dtype=np.uint8)
    depth = np.empty((P,) + rooms[0][1].shape, dtype=np.uint16)
    for i in range(P):
        r, turn = rooms[i % len(rooms)], (i // len(rooms)) * 61
        rgb[i], depth[i] = np.roll(r[0], turn, axis=1), np.roll(r[1], turn, axis=1)
    return rgb, depth


def planned_uploads(hyp, P: int, pool: int, B: int, epochs: int, policy: str):
    """Uploads per batch, per epoch, of a PanoCache with `policy` over the epochs a seed-0 train source runs ("ahead": furthest next use
    planned one batch ahead, the batch in flight kept -- what prefetch=True plans)."""
    ahead = policy == "ahead"
    cache = train_render.PanoCache(P, pool, B, policy="furthest" if ahead else policy, prefetch=ahead)
    gen = torch.Generator().manual_seed(0)
    out = []
    for _ in range(epochs):
        plan = train_render.plan_epoch(len(hyp), B, "train", gen)
        panos = [np.unique(np.concatenate([hyp.i1[idx], hyp.i2[idx]])) for idx in plan]
        next_use, after = train_render.epoch_next_use(panos, P)
        per = []
        for b, need in enumerate(panos):
            per.append(len(cache.plan(need, next_use, keep=panos[b - 1] if ahead and b else None)[1]))
            next_use[need] = after[b]
        out.append(per)
    return out


def sustained(a, tag, model, opt, x_packed, y, src_c, src_e, n_it) -> None:
    """Rows (c) and (e) and the resident batch over consecutive steps of whole epochs, the kinds alternating epoch by epoch (module docstring)."""
    kinds = {"resident": None, "(c) pool": src_c, "(e) pool + prefetch": src_e}
    steps, firsts, epochs, waits = ({k: [] for k in kinds} for _ in range(4))
    for r in range(1 + a.rounds):
        for k, src in kinds.items():
            it = None if src is None else iter(src)
            w0 = 0.0 if src is None else src.pool.wait_s
            torch.cuda.synchronize()
            t0 = t_prev = time.perf_counter()
            per = []
            for i in range(n_it):
                xb, yb = (x_packed, y) if it is None else next(it)
                opt.zero_grad(set_to_none=True)
                loss = F.cross_entropy(model.forward_packed(xb), yb.squeeze())
                loss.backward()
                opt.step()
                loss.item()   # (what training.run_epoch does every step: the compute stream is waited for, the copy stream is not)
                t = time.perf_counter()
                per.append(t - t_prev)
                t_prev = t
            if it is not None:
                for _ in it:   # (the status check behind the epoch)
                    pass
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            if r:   # the first round fills the pools
                steps[k] += per[1:]
                firsts[k].append(per[0])
                epochs[k].append(total / n_it)
                waits[k].append(0.0 if src is None else (src.pool.wait_s - w0) / (n_it - 1))
    res = med(steps["resident"]) * 1e3
    for k in kinds:
        m = med(steps[k]) * 1e3
        line = (f"{tag}: consecutive steps, {a.rounds} epochs of {n_it}: {k}: median step behind the first {m:.1f} ms ({100 * (m / res - 1):+.1f} % over the "
                f"resident step; min {min(steps[k]) * 1e3:.1f}, max {max(steps[k]) * 1e3:.1f}), first step of an epoch {med(firsts[k]) * 1e3:.1f} ms, epoch per batch "
                + " / ".join(f"{v * 1e3:.1f}" for v in epochs[k]) + " ms")
        if kinds[k] is not None and kinds[k].pool.prefetch:
            line += "; host wait for the upload job per prefetched batch " + " / ".join(f"{v * 1e3:.2f}" for v in waits[k]) + " ms"
        if kinds[k] is not None:
            line += f"; uploads so far {kinds[k].uploads}"
        print(line, flush=True)


def cache_rows(a, dev) -> None:
    """Rows (a)-(d) of DESIGN.md 4.11 (see the module docstring)."""
    B, n_it, P = a.batch, a.warmup + a.steps, a.panos
    if P < 4 * B:
        sys.exit(f"--panos {P}: the comparison of the feed's modes needs at least 4 x batch = {4 * B} panoramas")
    pool = a.resident_panos
    t0 = time.perf_counter()
    rgb, depth = distinct_panos(P)
    pano_bytes = rgb[0].nbytes + depth[0].nbytes
    print(f"# {torch.cuda.get_device_name(dev)}; batch {B}, {P} distinct synthetic 1024 x 512 panoramas ({time.perf_counter() - t0:.0f} s to make), "
          f"pool {pool}, an epoch = {n_it} batches, median of {a.steps} after {a.warmup} warm-up; step = forward + backward + Adam; rows alternate "
          "step by step", flush=True)
    hyp = synthetic.make_hypotheses(B * n_it, P)
    labels = np.arange(B * n_it, dtype=np.int64) % 2
    if pool is not None:
        for policy in ("furthest", "lru") + (("ahead",) if a.prefetch else ()):
            per = planned_uploads(hyp, P, pool, B, 3, policy)
            print(f"planned uploads per batch, {policy}: " + "; ".join(f"epoch {e + 1} mean {np.mean(v):.1f} (first batch {v[0]}, others {np.mean(v[1:]):.1f})"
                                                                       for e, v in enumerate(per)), flush=True)
    for cfg in a.configs.split(","):
        layers, nm = (int(v) for v in cfg.split(":"))
        for mode in a.modes.split(","):
            prec, norm = mode.split(":")
            tag = f"resnet{layers} {6 * nm}ch batch {B} {prec} norm {norm}"

            def make(**kw):
                s = train_render.RenderedTrainSource(dev, MODS[nm], batch_size=B, precision=prec, split="train", seed=0, **kw)
                t1 = time.perf_counter()
                s.load_panos(rgb, depth)
                torch.cuda.synchronize()
                print(f"{tag}: load_panos({kw or 'default'}) {time.perf_counter() - t1:.2f} s", flush=True)
                s.set_examples(hyp, labels)
                return s

            rows = {"(a) kept, all resident": make()}
            if a.identity == "batch" or pool is not None:
                rows["(b) batch, all resident"] = make(identity="batch")
            if pool is not None:
                rows["(d) pool, first epoch"] = make(identity="batch", resident_panos=pool)
            tags = ("upload", "index update", "scatter", "densify", "tiles")

            def alone(names, its):
                """Source alone: the named rows alternate batch by batch over one epoch each."""
                walls, splits = {k: [] for k in names}, {k: [] for k in names}
                for i in range(n_it):
                    for k in names:
                        src = rows[k]
                        src.timers = []
                        box = []
                        walls[k].append(wall(lambda: box.append(next(its[k]))))
                        sp = {t: 0.0 for t in tags}
                        for t, s0, e0 in src.timers:
                            sp[t] += s0.elapsed_time(e0)
                        splits[k].append(sp)
                        src.timers = None
                        last[k] = box[0]
                for k in names:
                    w = med(walls[k][a.warmup:]) * 1e3
                    sp = {t: med([s[t] for s in splits[k][a.warmup:]]) for t in tags}
                    line = f"{tag}: {k}: source alone {w:.2f} ms per batch (host clock); events: " + ", ".join(f"{t} {sp[t]:.2f}" for t in tags) + " ms"
                    if rows[k].pool is not None:
                        line += f"; uploads so far {rows[k].uploads}"
                    print(line, flush=True)
                    res_alone[k] = w

            last, res_alone = {}, {}
            random.seed(0)
            its = {k: iter(s) for k, s in rows.items()}
            pool_key = "(d) pool, first epoch"
            if pool is not None:
                u0 = rows[pool_key].uploads
            alone(list(rows), its)
            if pool is not None:   # the H2D rate of the cold epoch, and the same source's second epoch = row (c)
                src = rows[pool_key]
                for it in its.values():
                    for _ in it:   # (finish the epochs: the status check at their end)
                        pass
                cold = src.uploads - u0
                print(f"{tag}: cold epoch uploaded {cold} panoramas = {cold * pano_bytes / 1e9:.2f} GB", flush=True)
                rows["(c) pool, second epoch"] = rows.pop(pool_key)
                # per-batch upload events with their byte counts: the host-to-device rate actually reached
                rates = []
                src.timers = []
                it_c = iter(src)
                walls_c, splits_c = [], []
                for i in range(n_it):
                    del src.timers[:]
                    before = src.uploads
                    box = []
                    walls_c.append(wall(lambda: box.append(next(it_c))))
                    sp = {t: 0.0 for t in tags}
                    for t, s0, e0 in src.timers:
                        sp[t] += s0.elapsed_time(e0)
                    splits_c.append(sp)
                    m = src.uploads - before
                    if m and sp["upload"] > 0:
                        rates.append((m, m * pano_bytes / sp["upload"] / 1e6))
                    last["(c) pool, second epoch"] = box[0]
                src.timers = None
                w = med(walls_c[a.warmup:]) * 1e3
                sp = {t: med([s[t] for s in splits_c[a.warmup:]]) for t in tags}
                res_alone["(c) pool, second epoch"] = w
                print(f"{tag}: (c) pool, second epoch: source alone {w:.2f} ms per batch (host clock); events: " + ", ".join(f"{t} {sp[t]:.2f}" for t in tags) +
                      f" ms; uploads per batch {[m for m, _ in rates]}; host-to-device rate of the upload events (2 copies per batch, pinned) "
                      f"{[round(r, 1) for _, r in rates]} GB/s, median {med([r for _, r in rates]) if rates else float('nan'):.1f} GB/s", flush=True)
                for _ in it_c:
                    pass

            # ---- the step: resident packed batch, and fed by every row (the pool in its third epoch: steady), alternating
            torch.manual_seed(0)
            model = trainable.TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=MODS[nm])).to(dev).train()
            model.set_train_precision(prec).set_train_norm(norm)
            model = model.to(memory_format=torch.channels_last)
            opt = torch.optim.Adam(model.parameters(), lr=1e-4)
            x_packed, y = last["(a) kept, all resident"][0].clone(), last["(a) kept, all resident"][1].squeeze().clone()
            its = {k: iter(s) for k, s in rows.items()}
            res = {k: [] for k in ["resident"] + list(rows)}

            def fed(k):
                xb, yb = next(its[k])
                step(model, opt, lambda: model.forward_packed(xb), yb.squeeze())

            for i in range(n_it):
                res["resident"].append(wall(lambda: step(model, opt, lambda: model.forward_packed(x_packed), y)))
                for k in rows:
                    res[k].append(wall(lambda: fed(k)))
            m = {k: med(v[a.warmup:]) * 1e3 for k, v in res.items()}
            print(f"{tag}: step on a resident packed batch {m['resident']:.1f} ms; " +
                  "; ".join(f"fed by {k} {m[k]:.1f} ms ({100 * (m[k] / m['resident'] - 1):+.1f} %, source alone / resident step = "
                            f"{res_alone[k] / m['resident']:.3f})" for k in rows), flush=True)
            if pool is not None:   # the cold fill under the step: a fresh pool, its first epoch
                for it in its.values():
                    it.close()
                if a.prefetch:
                    sustained(a, tag, model, opt, x_packed, y, rows["(c) pool, second epoch"],
                              make(identity="batch", resident_panos=pool, prefetch=True, gather_threads=a.gather_threads), n_it)
                del rows["(c) pool, second epoch"]
                fresh = make(identity="batch", resident_panos=pool)
                it_d = iter(fresh)
                cold_fed, resident = [], []
                for i in range(n_it):
                    resident.append(wall(lambda: step(model, opt, lambda: model.forward_packed(x_packed), y)))

                    def fed_cold():
                        xb, yb = next(it_d)
                        step(model, opt, lambda: model.forward_packed(xb), yb.squeeze())

                    cold_fed.append(wall(fed_cold))
                r_, c_ = med(resident[a.warmup:]) * 1e3, med(cold_fed[a.warmup:]) * 1e3
                print(f"{tag}: (d) pool, first epoch: fed step {c_:.1f} ms beside the resident step {r_:.1f} ms ({100 * (c_ / r_ - 1):+.1f} %); its first batch "
                      f"(fills {min(pool, 2 * B)} slots at most) {cold_fed[0] * 1e3:.1f} ms", flush=True)
                it_d.close()
                del fresh
            else:
                for it in its.values():
                    it.close()
            del model, opt, rows, its, last, x_packed
            torch.cuda.empty_cache()


def layout_rows(a, dev) -> None:
    """The layout modality of the feed (see the module docstring)."""
    from salve_amd import layout, synthetic_layouts
    from salve_amd.common.sim2 import Sim2

    B, n_it, P = a.batch, a.warmup + a.steps, a.panos
    layouts = synthetic_layouts.make_layouts(P, seed=0)
    panos = synthetic.make_panos(P)
    rgb, depth = np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])
    hyp = synthetic.make_hypotheses(B * 3 * n_it, P)
    labels = np.arange(len(hyp), dtype=np.int64) % 2
    print(f"# {torch.cuda.get_device_name(dev)}; batch {B}, {P} synthetic panoramas with synthetic layouts ({int(layouts.room_count.sum())} room vertices, "
          f"{int(layouts.wdo_count.sum())} W/D/Os), median of {a.steps} after {a.warmup} warm-up; step = forward + backward + Adam, bf16 + hip norm; "
          "variants alternate step by step", flush=True)

    # ---- posing one batch: the existing host path against the device path, the same B posed + B identity layouts
    gen = torch.Generator().manual_seed(0)
    plan = train_render.plan_epoch(len(hyp), B, "train", gen)[:n_it]
    dl = layout.DeviceLayouts(layouts, dev, 2 * B)
    host, host_pack, dev_host, dev_event = [], [], [], []
    for idx in plan:
        def host_path():
            specs = [layouts.spec(int(hyp.i1[j]), Sim2(hyp.R[j], hyp.t[j], 1.0)) for j in idx] + [layouts.spec(int(hyp.i2[j])) for j in idx]
            t1 = time.perf_counter()
            packed = layout.pack_layouts(specs, dev)
            torch.cuda.synchronize()
            host_pack.append(time.perf_counter() - t1)
            return packed
        host.append(wall(host_path))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def device_path():
            recs = layout.pose_records(layouts, np.concatenate([hyp.i1[idx], hyp.i2[idx]]), np.concatenate([hyp.R[idx], hyp.R[idx]]),
                                       np.concatenate([hyp.t[idx], hyp.t[idx]]), None, np.arange(2 * B) < B)
            recs_dev = torch.from_numpy(recs.view(np.uint8)).to(dev)
            e0.record()
            dl.pose(recs_dev, 2 * B)
            e1.record()
        dev_host.append(wall(device_path))
        dev_event.append(e0.elapsed_time(e1))
    h, hp, d, de = (med(v[a.warmup:]) * 1e3 for v in (host, host_pack, dev_host, [x / 1e3 for x in dev_event]))
    print(f"posing 2 x {B} layouts: host path (specs + pack_layouts + upload) {h:.2f} ms per batch (pack_layouts + upload alone {hp:.2f} ms); device path "
          f"(records + upload + salve_layout_pose, host clock) {d:.3f} ms, its launch {de * 1e3:.1f} us (HIP events); host / device = {h / d:.0f} x", flush=True)
    del dl

    for layers, mods in ((50, ["layout"]), (152, ["ceiling_rgb_texture", "floor_rgb_texture", "layout"])):
        tag = f"resnet{layers} {6 * len(mods)}ch batch {B} bf16 norm hip"
        src = train_render.RenderedTrainSource(dev, mods, batch_size=B, precision="bf16", split="train", seed=0, layouts=layouts)
        src.load_panos(rgb, depth)
        src.set_examples(hyp, labels)
        random.seed(0)
        it = iter(src)
        src.timers, walls, splits = [], [], []
        for i in range(n_it):
            del src.timers[:]
            box = []
            walls.append(wall(lambda: box.append(next(it))))
            splits.append({t: s0.elapsed_time(e0) for t, s0, e0 in src.timers})
        src.timers = None
        x_packed, y = box[0][0].clone(), box[0][1].squeeze().clone()
        w = med(walls[a.warmup:]) * 1e3
        tags = [t for t in ("scatter", "densify", "layout pose", "layout rasterise", "tiles") if t in splits[0]]
        print(f"{tag}: source alone {w:.2f} ms per batch (host clock); events: " +
              ", ".join(f"{t} {med([s_[t] for s_ in splits[a.warmup:]]):.3f}" for t in tags) + " ms", flush=True)
        torch.manual_seed(0)
        model = trainable.TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=mods)).to(dev).train()
        model.set_train_precision("bf16").set_train_norm("hip")
        model = model.to(memory_format=torch.channels_last)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        res = {"resident": [], "fed": []}

        def fed():
            xb, yb = next(it)
            step(model, opt, lambda: model.forward_packed(xb), yb.squeeze())

        for i in range(n_it):
            res["resident"].append(wall(lambda: step(model, opt, lambda: model.forward_packed(x_packed), y)))
            res["fed"].append(wall(fed))
        m = {k: med(v[a.warmup:]) * 1e3 for k, v in res.items()}
        print(f"{tag}: step on a resident packed batch {m['resident']:.1f} ms ({B / m['resident'] * 1e3:.0f} samples/s); fed by the source {m['fed']:.1f} ms "
              f"({B / m['fed'] * 1e3:.0f} samples/s, {100 * (m['fed'] / m['resident'] - 1):+.1f} %); source alone / resident step = {w / m['resident']:.3f}",
              flush=True)
        it.close()
        del model, opt, src, x_packed
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="152:2,50:1", help="layers:surfaces, comma separated")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--modes", default="bf16:hip,fp32:torch", help="precision:norm, comma separated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--panos", type=int, default=64)
    ap.add_argument("--disk", type=int, default=0, help="batches of the end-to-end comparison with the on-disk path (0: skip)")
    ap.add_argument("--identity", choices=("kept", "batch"), default="kept", help="batch: compare the feed's modes (rows a, b) instead")
    ap.add_argument("--resident-panos", type=int, default=None, help="pool size: compare the feed's modes (rows a-d) instead; needs --panos >= 4 x batch")
    ap.add_argument("--prefetch", action="store_true", help="with --resident-panos N (N >= 4 x batch): add row (e), the pool with prefetch=True")
    ap.add_argument("--rounds", type=int, default=4, help="--prefetch: epochs of consecutive steps timed per kind (one more, the first, is dropped)")
    ap.add_argument("--gather-threads", type=int, default=4, help="--prefetch: host threads that gather the missed rows (1 .. 8)")
    ap.add_argument("--layout", action="store_true", help="the layout modality: device posing against the host path, ResNet-50 6ch and ResNet-152 18ch")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_train_feed.py needs the MI355X (a CPU run says nothing about it)")
    dev = torch.device("cuda:0")
    if a.prefetch and a.resident_panos is None:
        sys.exit("--prefetch belongs to --resident-panos N")
    if a.layout:
        layout_rows(a, dev)
        return
    if a.identity == "batch" or a.resident_panos is not None:
        cache_rows(a, dev)
        return
    B, n_it = a.batch, a.warmup + a.steps
    panos = synthetic.make_panos(a.panos)
    rgb, depth = np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])
    print(f"# {torch.cuda.get_device_name(dev)}; batch {B}, {a.panos} synthetic 1024 x 512 panoramas, median of {a.steps} after {a.warmup} warm-up; "
          "step = forward + backward + Adam; variants alternate step by step", flush=True)
    for cfg in a.configs.split(","):
        layers, nm = (int(v) for v in cfg.split(":"))
        for mode in a.modes.split(","):
            prec, norm = mode.split(":")
            n_ex = B * max(3 * n_it, a.disk)
            hyp = synthetic.make_hypotheses(n_ex, a.panos)
            labels = np.arange(n_ex, dtype=np.int64) % 2
            src = train_render.RenderedTrainSource(dev, MODS[nm], batch_size=B, precision=prec, split="train", seed=0)
            src.load_panos(rgb, depth)
            src.set_examples(hyp, labels)
            random.seed(0)
            tag = f"resnet{layers} {6 * nm}ch batch {B} {prec} norm {norm}"

            # ---- the source alone
            it = iter(src)
            src.timers, walls, splits = [], [], []
            for i in range(n_it):
                del src.timers[:]
                box = []
                walls.append(wall(lambda: box.append(next(it))))
                splits.append({t: s.elapsed_time(e) for t, s, e in src.timers})
            src.timers = None
            x_packed, y = box[0][0], box[0][1].squeeze()
            w = med(walls[a.warmup:]) * 1e3
            sp = {t: med([s[t] for s in splits[a.warmup:]]) for t in ("scatter", "densify", "tiles")}
            Hb, Wb = src.ras.bev_hw
            tile_bytes = x_packed.numel() * x_packed.element_size() + 2 * B * nm * Hb * Wb * 4
            print(f"{tag}: source alone {w:.2f} ms per batch (host clock); events: scatter {sp['scatter']:.2f}, densify {sp['densify']:.2f}, "
                  f"tile launch {sp['tiles']:.3f} ms = {tile_bytes / 1e9:.3f} GB of algorithmic bytes at {tile_bytes / sp['tiles'] / 1e9:.2f} TB/s "
                  f"({100 * tile_bytes / sp['tiles'] / 1e9 / COPY_TBS:.0f} % of the {COPY_TBS} TB/s copy rate)", flush=True)

            # ---- the step, three ways
            torch.manual_seed(0)
            model = trainable.TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=MODS[nm])).to(dev).train()
            model.set_train_precision(prec).set_train_norm(norm)
            model = model.to(memory_format=torch.channels_last)
            opt = torch.optim.Adam(model.parameters(), lr=1e-4)
            C = 6 * nm
            xs = [x_packed[..., 3 * k:3 * k + 3].permute(0, 3, 1, 2).float().contiguous() for k in range(2 * nm)]   # the same batch as NCHW fp32
            res = {"resident forward": [], "resident forward_packed": [], "fed forward_packed": []}

            def fed():
                xb, yb = next(it)
                step(model, opt, lambda: model.forward_packed(xb), yb.squeeze())

            for i in range(n_it):
                res["resident forward"].append(wall(lambda: step(model, opt, lambda: model(*xs), y)))
                res["resident forward_packed"].append(wall(lambda: step(model, opt, lambda: model.forward_packed(x_packed), y)))
                res["fed forward_packed"].append(wall(fed))
            m = {k: med(v[a.warmup:]) * 1e3 for k, v in res.items()}
            print(f"{tag}: step on resident NCHW inputs through forward {m['resident forward']:.1f} ms ({B / m['resident forward'] * 1e3:.0f} samples/s); "
                  f"resident packed input through forward_packed {m['resident forward_packed']:.1f} ms (cat + cast + pad copy: "
                  f"{m['resident forward'] - m['resident forward_packed']:+.1f} ms); fed by the source {m['fed forward_packed']:.1f} ms "
                  f"({B / m['fed forward_packed'] * 1e3:.0f} samples/s); feed / resident step = {w / m['resident forward']:.3f}", flush=True)
            it.close()

            # ---- end to end against the on-disk path
            if a.disk > 0:
                args = config(layers, nm, B)
                n_disk = a.disk * B
                tmp = Path(tempfile.mkdtemp(prefix="feed_zind_"))
                try:
                    write_zind_tree(tmp, src, n_disk)
                    args.data_root = str(tmp)
                    loader = training.get_dataloader(args, "train", seed=0)
                    sub = train_render.RenderedTrainSource(dev, MODS[nm], batch_size=B, precision=prec, split="train", seed=0)
                    sub.share_panos(src)
                    sub.set_examples(synthetic.HypothesisTable(hyp.i1[:n_disk], hyp.i2[:n_disk], hyp.R[:n_disk], hyp.t[:n_disk], hyp.theta_deg[:n_disk]),
                                     labels[:n_disk])
                    assert len(loader) == len(sub) == a.disk, (len(loader), len(sub))
                    t_r = wall(lambda: training.run_epoch(args, 0, model, sub, opt, "train"))
                    t_d = wall(lambda: training.run_epoch(args, 0, model, loader, opt, "train"))
                    print(f"{tag}: end to end over {a.disk} batches (run_epoch): rendered feed {n_disk / t_r:.0f} samples/s, on-disk path "
                          f"(JPEG decode + per-example transform, num_workers 0) {n_disk / t_d:.0f} samples/s", flush=True)
                finally:
                    shutil.rmtree(tmp, ignore_errors=True)
            del model, opt, xs, src, x_packed
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
