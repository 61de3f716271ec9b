"""salve_amd.train_files with read_ahead=True on the MI355X: the pipelined iteration yields the serial source's
batches bit for bit -- train and val, both entropy stages, both precisions, with files that take the host route among them -- raises
the serial source's errors at the serial source's batch, leaves a clean source behind an error or an abandoned iteration, and really
does read batches k + 1 and k + 2 before batch k is handed out.

The data set is the file's own: seven train (building 1208) and five val (building 0340) examples of 65 x 65 tiles in the
reference's naming, written with Pillow at quality 75; resize 40, crop 32, batch size 2: three batches per epoch, so the ring of
three fills and wraps.  Every comparison is torch.equal against the serial source built from the same list with the same seeds."""

import json
import random
import shutil
import threading
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import jpeg_cases as jc  # noqa: E402
from salve_amd import evaluate, jpeg, train_utils, training  # noqa: E402
from salve_amd import train as train_cli  # noqa: E402
from salve_amd.dataset.zind_data import ZindData  # noqa: E402
from salve_amd.train_files import TileFileLoader, TileFileSource  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402

DEV = torch.device("cuda:0")
BOTH = ("ceiling_rgb_texture", "floor_rgb_texture")
FLOOR = ("floor_rgb_texture",)
TILE, RESIZE, CROP = 65, 40, 32
SIZES = dict(resize_hw=(RESIZE, RESIZE), crop_hw=(CROP, CROP))


def config(data_root, modalities=BOTH, **kw) -> TrainingConfig:
    d = dict(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10, poly_lr_power=0.9,
             optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=False, resize_h=RESIZE, resize_w=RESIZE, train_h=CROP,
             train_w=CROP, apply_photometric_augmentation=False, modalities=tuple(modalities), cfg_stem="t", num_epochs=1,
             workers=0, batch_size=2, data_root=str(data_root), layout_data_root="", model_save_dirpath="")
    d.update(kw)
    return TrainingConfig(**d)


def _write_dataset(root: Path) -> Path:
    """Seven pairs of building 1208 (the train split) and five of building 0340 (the val split), alternating positive / negative, a
    ceiling and a floor tile for each panorama of a pair: discs and noise, no two alike."""
    from PIL import Image

    seed = 0
    for building, examples in (("1208", 7), ("0340", 5)):
        for i in range(examples):
            d = root / ("gt_alignment_approx" if i % 2 == 0 else "incorrect_alignment") / building
            d.mkdir(parents=True, exist_ok=True)
            for surface in ("ceiling", "floor"):
                for room, pano in ((4, 5), (7, 8)):
                    seed += 1
                    name = f"pair_{i}___door_0_0_rotated_{surface}_rgb_floor_01_partial_room_{room:02d}_pano_{pano}.jpg"
                    Image.fromarray(jc.make_image("disc" if seed % 3 else "noise", TILE, TILE, seed)).save(d / name, quality=75)
    return root


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    return _write_dataset(tmp_path_factory.mktemp("tiles_ahead") / "bev")


def _lists(root, modalities=BOTH):
    args = config(root, modalities)
    train, val = (ZindData(split=s, transform=None, args=args).data_list for s in ("train", "val"))
    assert (len(train), len(val)) == (7, 5)
    return train, val


def _source(data_list, read_ahead, split="train", cls=TileFileSource, **kw):
    return cls(DEV, data_list, batch_size=2, split=split, seed=3, read_ahead=read_ahead, **SIZES, **kw)


def _epochs(src, epochs, seed=11):
    """`epochs` whole iterations behind one random.seed: [[(x, y), ...], ...]."""
    random.seed(seed)
    return [list(src) for _ in range(epochs)]


def _assert_equal_batches(got, want):
    assert len(got) == len(want)
    for (x, y), (xw, yw) in zip(got, want):
        assert x.dtype == xw.dtype and x.shape == xw.shape and torch.equal(x, xw) and torch.equal(y, yw)


def _readers():
    return [t.name for t in threading.enumerate() if t.name.startswith("salve-tile-files")]


# ---------------------------------------------------------------------------------------------------- 1. equal batches
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("entropy", ["image", "lanes"])
@pytest.mark.parametrize("modalities", [BOTH, FLOOR], ids=["ceiling+floor", "floor"])
def test_read_ahead_yields_the_serial_batches(data_root, modalities, entropy, precision):
    train, val = _lists(data_root, modalities)
    out = {}
    for read_ahead in (False, True):
        with _source(train, read_ahead, entropy=entropy, precision=precision) as t, \
                _source(val, read_ahead, split="val", entropy=entropy, precision=precision) as v:
            assert len(t) == len(v) == 3
            out[read_ahead] = _epochs(t, 2) + _epochs(v, 1)
            assert t.fallbacks == v.fallbacks == 0 and t._epoch_status == [] and v._epoch_status == []
    for got, want in zip(out[True], out[False]):
        assert len(want) == 3
        _assert_equal_batches(got, want)
    assert [b[0].shape[0] for b in out[True][2]] == [2, 2, 1]                      # val: nothing dropped
    assert out[True][0][0][0].shape == (2, CROP, CROP, 8 * len(modalities))
    assert not torch.equal(out[False][0][0][0], out[False][1][0][0])               # (the second epoch is another shuffle, other draws)


# ---------------------------------------------------------------------------------------------------- 2. mixed routes
@pytest.mark.parametrize("entropy, fallbacks", [("image", 2), ("lanes", 1)])
def test_files_of_the_host_route_among_the_batch(data_root, tmp_path, entropy, fallbacks):
    from PIL import Image

    from salve_amd.utils import image_io

    root = tmp_path / "bev"
    shutil.copytree(data_root, root)
    train, _ = _lists(root)
    progressive, restarts = train[1][2], train[4][1]
    Image.fromarray(image_io.read_rgb(progressive)).save(progressive, format="JPEG", quality=75, progressive=True)
    Image.fromarray(image_io.read_rgb(restarts)).save(restarts, format="JPEG", quality=75, restart_marker_blocks=2)
    with pytest.raises(jpeg.Unsupported):
        jpeg.parse_file(Path(restarts).read_bytes())
    out = {}
    for read_ahead in (False, True):   # (split="val": in order, nothing dropped -- every file of the list is read)
        with _source(train, read_ahead, split="val", entropy=entropy) as src:
            out[read_ahead] = _epochs(src, 1)[0]
            assert src.fallbacks == fallbacks
    assert len(out[False]) == 4
    _assert_equal_batches(out[True], out[False])


# ---------------------------------------------------------------------------------------------------- 3. a malformed scan
@pytest.mark.parametrize("read_ahead", [False, True], ids=["serial", "read_ahead"])
def test_a_malformed_file_in_the_last_batch_is_named_at_the_end_of_the_epoch(data_root, tmp_path, read_ahead):
    root = tmp_path / "bev"
    shutil.copytree(data_root, root)
    _, val = _lists(root, FLOOR)
    victim = Path(val[4][0])                                                      # the last batch holds example 4 alone
    raw = victim.read_bytes()
    p = jpeg.parse_file(raw)
    victim.write_bytes(raw[:p.scan_offset + p.scan_bytes // 2] + raw[-2:])        # half the scan, the end marker still there
    got = []
    with _source(val, read_ahead, split="val") as src:
        with pytest.raises(RuntimeError, match=victim.name):
            for batch in src:
                got.append(batch)
        assert src._epoch_status == []
    assert len(got) == 3                                                          # every batch is yielded first
    _, val_good = _lists(data_root, FLOOR)
    with _source(val_good, False, split="val") as good:
        _assert_equal_batches(got[:2], list(good)[:2])


# ---------------------------------------------------------------------------------------------------- 4. a missing file
def test_a_missing_file_raises_at_its_batch_and_the_source_restarts_clean(data_root, tmp_path):
    root = tmp_path / "bev"
    shutil.copytree(data_root, root)
    train, _ = _lists(root)
    before = _readers()
    with _source(train, False, split="val") as serial:
        want = _epochs(serial, 1)[0]
    victim = Path(train[2][3])                                                    # batch 1 holds examples 2 and 3
    away = victim.with_suffix(".away")
    victim.rename(away)
    src = _source(train, True, split="val")
    got = []
    with pytest.raises(FileNotFoundError, match=victim.name):
        for batch in src:
            got.append(batch)
    _assert_equal_batches(got, want[:1])                                          # the batch before it is yielded, none behind it
    assert src._epoch_status == [] and src._ahead == {}
    away.rename(victim)
    _assert_equal_batches(_epochs(src, 1)[0], want)
    assert any(n.startswith("salve-tile-files-pack") for n in _readers())
    src.close()
    assert _readers() == before
    _assert_equal_batches(_epochs(src, 1)[0], want)                               # usable after close(): new threads
    src.close()
    assert _readers() == before


# ---------------------------------------------------------------------------------------------------- 5. an abandoned iteration
def test_an_abandoned_iteration_leaves_the_serial_sources_state(data_root):
    train, _ = _lists(data_root)
    out = {}
    for read_ahead in (False, True):
        with _source(train, read_ahead) as src:
            random.seed(5)
            it = iter(src)
            first = next(it)
            it.close()
            del it
            if read_ahead:
                assert src._ahead == {} and src._epoch_status == []
            out[read_ahead] = [first] + list(src) + list(src)
    assert len(out[False]) == 7
    _assert_equal_batches(out[True], out[False])


# ---------------------------------------------------------------------------------------------------- 6. the overlap, without a clock
class _Logged(TileFileSource):
    """Logs ("read", j) when `_read` is entered for the epoch's j-th batch; the consumer appends ("yield", k)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.log, self.reads = [], 0

    def _read(self, paths):
        self.log.append(("read", self.reads))
        self.reads += 1
        return super()._read(paths)


@pytest.mark.parametrize("read_ahead", [False, True], ids=["serial", "read_ahead"])
def test_the_next_batches_are_read_before_the_current_one_is_yielded(data_root, read_ahead):
    train, _ = _lists(data_root)
    with _source(train, read_ahead, split="val", cls=_Logged) as src:
        for k, _ in enumerate(src):
            src.log.append(("yield", k))
        log = list(src.log)
    at = {entry: i for i, entry in enumerate(log)}
    assert len(log) == 8 and sorted(at) == sorted([("read", j) for j in range(4)] + [("yield", k) for k in range(4)])
    for k in range(4):
        assert at["read", k] < at["yield", k]
        for ahead in (k + 1, k + 2):
            if ahead < 4:
                if read_ahead:
                    assert at["read", ahead] < at["yield", k], (k, ahead, log)
                else:
                    assert at["read", ahead] > at["yield", k], (k, ahead, log)
        if k + 3 < 4:
            assert at["read", k + 3] > at["yield", k], (k, log)                   # two ahead, not three: the ring has three slots


# ---------------------------------------------------------------------------------------------------- 7. the evaluation loader
def _loader(data_list, read_ahead, batch_size=2, **kw):
    return TileFileLoader(DEV, data_list, batch_size, (RESIZE, RESIZE), (CROP, CROP), read_ahead=read_ahead, **kw)


@pytest.mark.parametrize("entropy", ["image", "lanes"])
@pytest.mark.parametrize("modalities", [BOTH, FLOOR], ids=["ceiling+floor", "floor"])
def test_evaluation_loader_yields_the_serial_loaders_tuples(data_root, modalities, entropy):
    _, val = _lists(data_root, modalities)
    with _loader(val, False, entropy=entropy) as serial, _loader(val, True, entropy=entropy) as ahead:
        want, got = list(serial), list(ahead)
    assert len(want) == len(got) == 3
    for a, b in zip(want, got):
        assert len(a) == len(b) == 2 * len(modalities) + 3
        *xa, ya, fa0, fa1 = a
        *xb, yb, fb0, fb1 = b
        for u, v in zip(xa, xb):
            assert v.dtype == torch.float32 and v.shape == u.shape and torch.equal(u, v)
        assert torch.equal(ya, yb) and fa0 == fb0 and fa1 == fb1
    ahead = train_utils.get_dataloader(config(data_root, modalities), "val", decode="device", entropy=entropy, read_ahead=True)
    assert isinstance(ahead, TileFileLoader) and ahead.read_ahead and len(ahead.data_list) == 5
    assert not train_utils.get_dataloader(config(data_root, modalities), "val", decode="device").read_ahead


def test_run_test_epoch_writes_identical_prediction_files(data_root, tmp_path):
    """The inference engine is compiled for 224 x 224 tiles and takes no other size: the same 65 x 65 files, resized to 234 and
    cropped to 224 here."""
    args = config(data_root, batch_size=3, resize_h=234, resize_w=234, train_h=224, train_w=224)   # (batches of 3 + 2: the loss refuses ONE example)
    _, val = _lists(data_root)
    torch.manual_seed(0)
    model = train_utils.get_model(args)
    full = lambda read_ahead: TileFileLoader(DEV, val, 3, (234, 234), (224, 224), read_ahead=read_ahead)
    with full(False) as serial, full(True) as ahead:
        m_serial = evaluate.run_test_epoch(args, str(tmp_path / "serial"), "ckpt.pth", model, serial, "test")
        m_ahead = evaluate.run_test_epoch(args, str(tmp_path / "ahead"), "ckpt.pth", model, ahead, "test")
    assert m_serial == m_ahead
    names = sorted(p.name for p in (tmp_path / "serial").iterdir())
    assert names == ["batch_0.json", "batch_1.json"] == sorted(p.name for p in (tmp_path / "ahead").iterdir())
    for name in names:
        assert (tmp_path / "serial" / name).read_bytes() == (tmp_path / "ahead" / name).read_bytes()
    assert len(json.loads((tmp_path / "ahead" / "batch_1.json").read_text())["y_true"]) == 2


# ---------------------------------------------------------------------------------------------------- 8. one tiny epoch
def test_one_tiny_training_epoch_with_read_ahead(data_root, tmp_path):
    args = config(data_root, batch_size=3)   # two train batches (building 1208), val batches of 3 + 2 (0340)
    before = _readers()
    serial = training.train(args, str(tmp_path / "serial"), seed=0, decode="device")
    res = training.train(args, str(tmp_path / "ahead"), seed=0, decode="device", read_ahead=True)
    assert _readers() == before
    assert set(res) == set(serial) == {"train_avg_loss", "train_mAcc", "val_avg_loss", "val_mAcc"}
    assert all(len(res[k]) == len(serial[k]) == 1 for k in res) and np.isfinite(res["train_avg_loss"][0])
    ck = torch.load(tmp_path / "ahead" / "train_ckpt.pth", map_location="cpu", weights_only=False)
    from salve_amd.models.trainable import TrainableEarlyFusionCEResnet

    TrainableEarlyFusionCEResnet(18, False, 2, args).load_state_dict(ck["state_dict"], strict=True)
    on_disk = json.loads((tmp_path / "ahead" / "results-t.json").read_text())
    assert set(on_disk) == set(serial) and all(len(v) == 1 for v in on_disk.values())


def test_the_cli_flag_trains_one_tiny_epoch(data_root, tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("TrainingConfig:\n    _target_: salve.training_config.TrainingConfig\n    lr_annealing_strategy: poly\n    base_lr: 0.001\n"
                   "    weight_decay: 0.0001\n    num_ce_classes: 2\n    print_every: 10\n    poly_lr_power: 0.9\n    optimizer_algo: adam\n"
                   f"    num_layers: 18\n    pretrained: False\n    dataparallel: True\n    resize_h: {RESIZE}\n    resize_w: {RESIZE}\n"
                   f"    train_h: {CROP}\n    train_w: {CROP}\n    apply_photometric_augmentation: False\n"
                   "    modalities: [\"ceiling_rgb_texture\", \"floor_rgb_texture\"]\n"
                   "    cfg_stem: ahead\n    num_epochs: 50\n    workers: 15\n    batch_size: 256\n    data_root: /nonexistent\n    layout_data_root:\n"
                   f"    model_save_dirpath: {tmp_path / 'models'}\n    gpu_ids:\n")
    out = tmp_path / "run"
    before = _readers()
    train_cli.main(["--config", str(cfg), "--epochs", "1", "--batch-size", "3", "--data-root", str(data_root), "--seed", "0", "--out", str(out),
                    "--decode", "device", "--decode-read-ahead", "--decode-entropy", "lanes", "--precision", "bf16"])
    assert _readers() == before
    ck = torch.load(out / "train_ckpt.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "max_epochs", "curr_val_mAcc", "best_so_far_val_mAcc"} and ck["max_epochs"] == 1
    res = json.loads((out / "results-ahead.json").read_text())
    assert set(res) == {"train_avg_loss", "train_mAcc", "val_avg_loss", "val_mAcc"} and all(len(v) == 1 for v in res.values())
