"""salve_amd.train_files on the MI355X: batches from the tile data set on disk, decoded on the device, equal -- bit for bit -- what
the host route (Pillow + TrainTransform / the evaluation DataLoader) makes of the same files; the Pillow fallback for a file the
device does not decode; a malformed file named at the end of the epoch; `run_test_epoch`'s prediction files; one tiny
`train(decode="device")` epoch."""

import json
import random
import shutil
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import evaluate, jpeg, train_utils, training  # noqa: E402
from salve_amd.dataset.zind_data import ZindData  # noqa: E402
from salve_amd.train_files import TileFileLoader, TileFileSource  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

DEV = torch.device("cuda:0")
RENDERINGS = Path(__file__).resolve().parent / "golden" / "renderings"
BOTH = ("ceiling_rgb_texture", "floor_rgb_texture")


def config(data_root, modalities=BOTH, **kw) -> TrainingConfig:
    d = dict(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10, poly_lr_power=0.9,
             optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=False, resize_h=234, resize_w=234, train_h=224,
             train_w=224, apply_photometric_augmentation=False, modalities=tuple(modalities), cfg_stem="t", num_epochs=1,
             workers=0, batch_size=2, data_root=str(data_root), layout_data_root="", model_save_dirpath="")
    d.update(kw)
    return TrainingConfig(**d)


def _write_dataset(root: Path) -> Path:
    """The fixture pair as the positive example and two pairs written with image_io.write_jpeg as negatives, in the reference's
    naming; building 1208 is of the train split, 0340 of the val split."""
    src = RENDERINGS / "gt_alignment_approx" / "1208"
    for building in ("1208", "0340"):
        pos, neg = root / "gt_alignment_approx" / building, root / "incorrect_alignment" / building
        pos.mkdir(parents=True)
        neg.mkdir(parents=True)
        for f in src.glob("*.jpg"):
            shutil.copy(f, pos / f.name)
            rgb = image_io.read_rgb(str(f))
            image_io.write_jpeg(str(neg / f.name.replace("pair_58", "pair_3")), rgb[::-1].copy())
            image_io.write_jpeg(str(neg / f.name.replace("pair_58", "pair_7")), rgb[:, ::-1].copy())
    return root


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    return _write_dataset(tmp_path_factory.mktemp("tiles") / "bev")


def _host_batch(data_list, idx, draws, resize_crop=((234, 234), (224, 224))):
    """The host route: Pillow decodes every file, TrainTransform.apply with the given draws, repacked to the stem's NHWC input."""
    from salve_amd.transforms import TrainTransform

    tf = TrainTransform(*resize_crop, device=DEV)
    rows = []
    for i, draw in zip(idx, draws):
        *paths, _ = data_list[int(i)]
        tiles = tf.apply(tuple(image_io.read_rgb(p) for p in paths), *draw)
        x = torch.cat(tiles, 0).permute(1, 2, 0)                      # [crop, crop, 3 * images]
        rows.append(torch.nn.functional.pad(x, (0, (x.shape[2] + 7) // 8 * 8 - x.shape[2])))
    return torch.stack(rows), torch.tensor([[int(data_list[int(i)][-1])] for i in idx], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("modalities", [BOTH, ("floor_rgb_texture",)], ids=["ceiling+floor", "floor"])
def test_batch_equals_the_host_route_bit_for_bit(data_root, modalities):
    import threading

    readers = lambda: sum(t.name.startswith("salve-tile-files") for t in threading.enumerate())
    before = readers()
    data = ZindData(split="train", transform=None, args=config(data_root, modalities))
    assert len(data.data_list) == 3
    idx = np.array([2, 0, 1])
    draws = [(0, 10, False, True), (7, 3, True, False), (10, 0, True, True)]
    want, labels = _host_batch(data.data_list, idx, draws)
    src = TileFileSource(DEV, data.data_list, batch_size=3, split="train")
    x, y = src.batch(idx, draws)
    assert x.dtype == torch.float32 and x.shape == (3, 224, 224, 8 * len(modalities)) and x.is_contiguous()
    assert torch.equal(x, want) and torch.equal(y, labels)
    assert src.fallbacks == 0
    bf = TileFileSource(DEV, data.data_list, batch_size=3, split="train", precision="bf16")
    xb, _ = bf.batch(idx, draws)
    assert xb.dtype == torch.bfloat16 and torch.equal(xb, want.to(torch.bfloat16))   # the same rounding: nearest even
    src._check_epoch("test")
    bf._check_epoch("test")
    assert readers() > before
    src.close()
    bf.close()
    assert readers() == before and src._pool is None          # close() ends the reader threads ...
    with src:
        x2, _ = src.batch(idx, draws)                     # ... and the source stays usable: the next batch starts new ones
        assert torch.equal(x2, x) and readers() > before
    assert readers() == before


def test_iteration_follows_the_dataloaders_order_and_draws(data_root):
    args = config(data_root)
    data = ZindData(split="train", transform=None, args=args)
    src = TileFileSource(DEV, data.data_list, batch_size=2, split="train", seed=3)
    assert len(src) == 1
    random.seed(11)
    got = list(src)
    gen = torch.Generator()
    gen.manual_seed(3)
    order = [b.numpy() for b in torch.utils.data.DataLoader(range(3), batch_size=2, shuffle=True, generator=gen, drop_last=True)]
    random.seed(11)
    draws = [src.tf.draw() for _ in range(2)]
    want, labels = _host_batch(data.data_list, order[0], draws)
    assert len(got) == 1 and torch.equal(got[0][0], want) and torch.equal(got[0][1], labels)
    val = TileFileSource(DEV, data.data_list, batch_size=2, split="val")
    batches = list(val)
    assert [b[0].shape[0] for b in batches] == [2, 1]                  # in order, nothing dropped, the centre crop
    want, _ = _host_batch(data.data_list, [0, 1, 2], [(5, 5, False, False)] * 3)
    assert torch.equal(torch.cat([b[0] for b in batches]), want)


def test_a_progressive_file_takes_the_host_route(data_root, tmp_path):
    from PIL import Image

    root = tmp_path / "bev"
    shutil.copytree(data_root, root)
    data = ZindData(split="train", transform=None, args=config(root))
    victim = data.data_list[1][2]
    Image.fromarray(image_io.read_rgb(victim)).save(victim, format="JPEG", quality=75, progressive=True)
    with pytest.raises(jpeg.Unsupported):
        jpeg.parse_file(Path(victim).read_bytes())
    idx, draws = np.array([0, 1, 2]), [(1, 2, True, False), (3, 4, False, False), (9, 9, False, True)]
    want, _ = _host_batch(data.data_list, idx, draws)
    src = TileFileSource(DEV, data.data_list, batch_size=3, split="train")
    x, _ = src.batch(idx, draws)
    assert src.fallbacks == 1 and torch.equal(x, want)
    src._check_epoch("test")


def test_a_malformed_file_is_named_at_the_end_of_the_epoch(data_root, tmp_path):
    root = tmp_path / "bev"
    shutil.copytree(data_root, root)
    data = ZindData(split="train", transform=None, args=config(root, ("floor_rgb_texture",)))
    victim = Path(data.data_list[2][0])
    raw = victim.read_bytes()
    p = jpeg.parse_file(raw)
    victim.write_bytes(raw[:p.scan_offset + p.scan_bytes // 2] + raw[-2:])   # half the scan, the end marker still there
    src = TileFileSource(DEV, data.data_list, batch_size=2, split="val")
    with pytest.raises(RuntimeError, match=victim.name):
        for _ in src:
            pass


def _loaders(data_root, modalities=BOTH, batch_size=2):
    args = config(data_root, modalities, batch_size=batch_size)
    # (building 1208 is of the train split, for which get_dataloader refuses: the loader it builds for val / test, over those tiles)
    data = ZindData(split="train", transform=train_utils.get_val_test_transform(args), args=args)
    host = torch.utils.data.DataLoader(data, batch_size=args.batch_size, shuffle=False, num_workers=0, drop_last=False)
    device = TileFileLoader(DEV, data.data_list, args.batch_size, (args.resize_h, args.resize_w), (args.train_h, args.train_w))
    return args, host, device


@pytest.mark.parametrize("modalities", [BOTH, ("ceiling_rgb_texture",)], ids=["ceiling+floor", "ceiling"])
def test_evaluation_loader_yields_the_dataloaders_tuples(data_root, modalities):
    args, host, device = _loaders(data_root, modalities)
    assert len(host) == len(device) == 2
    for a, b in zip(host, device):
        assert len(a) == len(b) == 2 * len(modalities) + 3
        *xa, ya, fa0, fa1 = a
        *xb, yb, fb0, fb1 = b
        for u, v in zip(xa, xb):
            assert v.dtype == torch.float32 and v.device == u.device and torch.equal(u, v)
        assert ya.dtype == yb.dtype and torch.equal(ya, yb) and list(fa0) == list(fb0) and list(fa1) == list(fb1)
    val = train_utils.get_dataloader(config(data_root), "val", decode="device")   # building 0340
    assert isinstance(val, TileFileLoader) and len(val.data_list) == 3
    with pytest.raises(ValueError):
        train_utils.get_dataloader(config(data_root), "val", decode="gpu")


def test_run_test_epoch_writes_identical_prediction_files(data_root, tmp_path):
    args, host, device = _loaders(data_root, batch_size=3)   # (a last batch of ONE example is refused by the loss, whoever loads it)
    torch.manual_seed(0)
    model = train_utils.get_model(args)
    m_host = evaluate.run_test_epoch(args, str(tmp_path / "host"), "ckpt.pth", model, host, "test")
    m_dev = evaluate.run_test_epoch(args, str(tmp_path / "device"), "ckpt.pth", model, device, "test")
    assert m_host == m_dev
    assert sorted(p.name for p in (tmp_path / "device").iterdir()) == ["batch_0.json"]
    assert (tmp_path / "host" / "batch_0.json").read_bytes() == (tmp_path / "device" / "batch_0.json").read_bytes()
    assert json.loads((tmp_path / "device" / "batch_0.json").read_text())["y_true"] == [1, 0, 0]


def test_one_tiny_training_epoch_from_device_decoded_files(data_root, tmp_path):
    args = config(data_root, batch_size=3)   # one train batch (building 1208) and one val batch (0340) of three examples
    res = training.train(args, str(tmp_path / "run"), seed=0, decode="device")
    assert set(res) == {"train_avg_loss", "train_mAcc", "val_avg_loss", "val_mAcc"} and all(len(v) == 1 for v in res.values())
    assert np.isfinite(res["train_avg_loss"][0])
    ck = torch.load(tmp_path / "run" / "train_ckpt.pth", map_location="cpu", weights_only=False)
    from salve_amd.models.trainable import TrainableEarlyFusionCEResnet

    TrainableEarlyFusionCEResnet(18, False, 2, args).load_state_dict(ck["state_dict"], strict=True)
    with pytest.raises(ValueError):
        training.train(args, str(tmp_path / "bad"), decode="gpu")
