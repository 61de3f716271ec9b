"""Host side of the rendered training feed (salve_amd.train_render, salve_bev_train_tiles, forward_packed): the export and the
ctypes struct, epoch order and augmentation draws against a real DataLoader / TrainTransform.draw, and the refusals that need no GPU."""

import ctypes
import json
import random
import re
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from salve_amd import _lib, synthetic, train_render  # noqa: E402
from salve_amd.models.trainable import TrainableEarlyFusionCEResnet  # noqa: E402
from salve_amd.transforms import TrainTransform  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "salve_hip.h").read_text()
FLOOR, BOTH = ["floor_rgb_texture"], ["ceiling_rgb_texture", "floor_rgb_texture"]


# ---------------------------------------------------------------------------------------------------- 1. library
def test_library_exports_train_tiles_and_abi_stays_7():
    lib = _lib.load()
    assert hasattr(lib, "salve_bev_train_tiles") and "salve_bev_train_tiles" in _lib.EXPORTED_SYMBOLS
    assert re.search(r"\bint salve_bev_train_tiles\(", HEADER)
    assert lib.salve_hip_version() == 7 == _lib.EXPECTED_ABI
    assert int(re.search(r"#define SALVE_HIP_ABI_VERSION (\d+)", HEADER).group(1)) == 7


def test_draw_struct_has_the_headers_size():
    # salve_tile_aug_t in the header: four int32 fields; the numpy dtype the host packs the per-sample draws with must match it
    body = re.search(r"typedef struct \{([^}]*)\} salve_tile_aug_t;", HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("int32_t", "").split(",")]
    assert names == ["crop_y", "crop_x", "flags", "reserved"]

    class Aug(ctypes.Structure):
        _fields_ = [(n, ctypes.c_int32) for n in names]

    assert _lib.TILE_AUG_DTYPE.itemsize == ctypes.sizeof(Aug) == 16 and list(_lib.TILE_AUG_DTYPE.names) == names
    for name, value in (("SALVE_TILE_F32_NHWC", _lib.TILE_F32_NHWC), ("SALVE_TILE_BF16_NHWC", _lib.TILE_BF16_NHWC),
                        ("SALVE_STATUS_BAD_TILE_JOB", _lib.STATUS_BAD_TILE_JOB)):
        assert int(re.search(rf"#define {name} (\d+)", HEADER).group(1)) == value


# ---------------------------------------------------------------------------------------------------- 2. order and draws
def _loader(n, batch, seed):
    gen = torch.Generator()
    gen.manual_seed(seed)   # as training.get_dataloader seeds it
    return torch.utils.data.DataLoader(range(n), batch_size=batch, shuffle=True, generator=gen, num_workers=0, drop_last=True)


@pytest.mark.parametrize("n,batch,seed", [(40, 16, 0), (35, 8, 7), (16, 16, 3), (11, 4, 1)])
def test_train_order_is_the_dataloaders(n, batch, seed):
    loader = _loader(n, batch, seed)
    gen = torch.Generator()
    gen.manual_seed(seed)
    for epoch in range(3):   # the generator's state carries over from epoch to epoch, as the loader's does
        want = [b.tolist() for b in loader]
        got = [b.tolist() for b in train_render.plan_epoch(n, batch, "train", gen)]
        assert got == want and len(got) == n // batch, (epoch, got, want)
    other = torch.Generator()
    other.manual_seed(seed + 1)
    assert [b.tolist() for b in train_render.plan_epoch(n, batch, "train", other)] != want


def test_val_order_and_short_last_batch():
    got = train_render.plan_epoch(11, 4, "val")
    assert [b.tolist() for b in got] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]


@pytest.mark.parametrize("n", [0, 15, 16, 35])   # N = 0, B - 1, B, 2 B + 3
def test_batches_per_epoch(n):
    B = 16
    gen = torch.Generator()
    gen.manual_seed(0)
    assert train_render.batches_per_epoch(n, B, "train") == len(train_render.plan_epoch(n, B, "train", gen)) == n // B
    assert train_render.batches_per_epoch(n, B, "val") == len(train_render.plan_epoch(n, B, "val")) == -(-n // B)
    val = train_render.plan_epoch(n, B, "val")
    assert sum(len(b) for b in val) == n and all(len(b) == B for b in val[:-1])


class _PlanOnly(train_render.RenderedTrainSource):
    """The source's planning part without a device (no rasteriser, no panoramas)."""

    def __init__(self, split, resize=234, crop=224):
        self.split, self.tf = split, TrainTransform((resize, resize), (crop, crop))


def test_draws_are_train_transform_draws():
    B, s = 16, 5
    random.seed(s)
    got = _PlanOnly("train").draws(B)
    tf = TrainTransform((234, 234), (224, 224))
    random.seed(s)
    assert got == [tf.draw() for _ in range(B)]
    assert len({d[:2] for d in got}) > 1 and {d[2] for d in got} == {True, False}
    assert _PlanOnly("val").draws(3) == [(5, 5, False, False)] * 3   # ValTestTransform: centre crop, no flips


# ---------------------------------------------------------------------------------------------------- 3. refusals
def test_layout_modality_is_refused():
    for mods in (["layout"], BOTH + ["layout"]):
        with pytest.raises(RuntimeError, match="layout"):
            train_render.RenderedTrainSource("cuda:0", mods)


def test_batch_times_surfaces_over_the_library_limit_is_refused():
    with pytest.raises(RuntimeError, match="65535"):
        train_render.RenderedTrainSource("cuda:0", BOTH, batch_size=32768)
    with pytest.raises(RuntimeError, match="65535"):
        train_render.RenderedTrainSource("cuda:0", FLOOR, batch_size=65536)
    train_render.check_launch(32767, 2)
    train_render.check_launch(65535, 1)


def test_example_table_checks():
    hyp = synthetic.make_hypotheses(10, 4)
    ok = train_render.plan_examples(hyp, np.arange(10) % 2, 4)
    assert ok["is_match"].dtype == np.int64 and ok["swap"].tolist() == [0] * 10
    with pytest.raises(RuntimeError, match="one label per hypothesis"):
        train_render.plan_examples(hyp, np.zeros(9, dtype=np.int64), 4)
    with pytest.raises(RuntimeError, match="panorama"):
        train_render.plan_examples(hyp, np.zeros(10, dtype=np.int64), int(max(hyp.i1.max(), hyp.i2.max())))   # one panorama short
    bad = synthetic.make_hypotheses(10, 4)
    bad.i2 = bad.i2.copy()
    bad.i2[3] = -1
    with pytest.raises(RuntimeError, match="i2 names panorama -1"):
        train_render.plan_examples(bad, np.zeros(10, dtype=np.int64), 4)


def test_render_from_with_a_missing_file_is_one_line(tmp_path):
    np.save(tmp_path / "panos_rgb.npy", np.zeros((1, 8, 16, 3), dtype=np.uint8))
    np.save(tmp_path / "panos_depth.npy", np.zeros((1, 8, 16), dtype=np.uint16))
    (tmp_path / "train.json").write_text(json.dumps({"i1": [], "i2": [], "R": [], "t": [], "is_match": []}))
    with pytest.raises(SystemExit, match="val.json is missing"):
        train_render.load_render_dir(str(tmp_path))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("TrainingConfig:\n    lr_annealing_strategy: poly\n    base_lr: 0.001\n    weight_decay: 0.0001\n    num_ce_classes: 2\n"
                   "    print_every: 10\n    poly_lr_power: 0.9\n    optimizer_algo: adam\n    num_layers: 18\n    pretrained: False\n"
                   "    dataparallel: True\n    resize_h: 234\n    resize_w: 234\n    train_h: 224\n    train_w: 224\n"
                   "    apply_photometric_augmentation: False\n    modalities: [\"floor_rgb_texture\"]\n    cfg_stem: t\n    num_epochs: 1\n"
                   "    workers: 0\n    batch_size: 2\n    data_root: /nonexistent\n    layout_data_root:\n    model_save_dirpath: /nonexistent\n")
    r = subprocess.run([sys.executable, "-m", "salve_amd.train", "--config", str(cfg), "--render-from", str(tmp_path), "--out", str(tmp_path / "o")],
                       cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "Traceback" not in r.stderr
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert "val.json is missing" in lines[-1] and sum("missing" in ln for ln in lines) == 1, r.stderr


# ---------------------------------------------------------------------------------------------------- 4. forward_packed arguments
@pytest.mark.parametrize("mods,cp", [(FLOOR, 8), (BOTH, 16)])
def test_forward_packed_refuses_wrong_dtype_and_channels(mods, cp):
    model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=mods))
    with pytest.raises(RuntimeError, match=rf"\[B, H, W, {cp}\]"):
        model.forward_packed(torch.zeros(1, 8, 8, cp + 8))
    with pytest.raises(RuntimeError, match=rf"\[B, H, W, {cp}\]"):
        model.forward_packed(torch.zeros(1, 8, 8, cp - 2))
    with pytest.raises(RuntimeError, match="takes torch.float32, got torch.bfloat16"):
        model.forward_packed(torch.zeros(1, 8, 8, cp, dtype=torch.bfloat16))
    model.set_train_precision("bf16")
    with pytest.raises(RuntimeError, match="takes torch.bfloat16, got torch.float32"):
        model.forward_packed(torch.zeros(1, 8, 8, cp, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="HIP device only"):   # right shape and dtype: refused for the device, never run on the CPU
        model.forward_packed(torch.zeros(1, 8, 8, cp, dtype=torch.bfloat16))
