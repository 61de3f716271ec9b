"""The pair-overlap case list and its numpy emulator (tests/overlap_cases.py), checked on the host: the emulator is the reference's
texture_map_iou (salve/utils/iou_utils.py:14-37) restated from its definition, the case list covers what the issue of this kernel names,
and every emulated WRONG kernel fails at least one case -- so a GPU kernel with that mistake cannot pass tests/test_gpu_pair_overlap.py."""

import numpy as np
import pytest

from tests import overlap_cases as oc


def texture_map_iou(f1: np.ndarray, f2: np.ndarray) -> float:
    """iou_utils.py:14-37 from its definition: occupied = the largest channel is positive; |and| / (|or| + 1e-12)."""
    m1, m2 = np.amax(f1, axis=2) > 0, np.amax(f2, axis=2) > 0
    return np.logical_and(m1, m2).sum() / (np.logical_or(m1, m2).sum() + 1e-12)


def pack(rgb: np.ndarray) -> np.ndarray:
    """uint8 [h, w, 3] -> uint32 [1, h, w] 0x00BBGGRR, as the rasteriser holds an image."""
    c = rgb.astype(np.uint32)
    return (c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16))[None]


def reference_pairs():
    """The two cases of the reference's tests/utils/test_iou_utils.py, as data: (f1, f2, expected IoU)."""
    f1 = np.zeros((2, 2, 3), dtype=np.uint8)
    f1[0, 0], f1[1, 1] = [0, 100, 0], [100, 0, 0]
    f2 = np.zeros((2, 2, 3), dtype=np.uint8)
    f2[0, 0], f2[1, 0] = [0, 0, 100], [0, 100, 0]
    m1 = np.array([[1, 0, 0], [1, 1, 0], [1, 1, 1]], dtype=np.uint8)
    m2 = np.array([[0, 0, 1], [0, 1, 1], [0, 0, 0]], dtype=np.uint8)
    grey = lambda m: np.repeat((m * 37)[..., None], 3, axis=2)
    return [(f1, f2, 1 / 3), (grey(m1), grey(m2), 1 / 8)]


@pytest.mark.parametrize("k", [0, 1])
def test_emulator_equals_texture_map_iou_on_the_reference_cases(k):
    f1, f2, want = reference_pairs()[k]
    out = np.zeros((1, 4), dtype=np.int32)
    assert not oc.emulate(pack(f1), pack(f2), f1.shape[0], f1.shape[1], [0], [0], out)
    inter, union, na, nb = out[0].tolist()
    assert inter / (union + 1e-12) == texture_map_iou(f1, f2)
    assert np.isclose(inter / (union + 1e-12), want)
    assert na == int((np.amax(f1, axis=2) > 0).sum()) and nb == int((np.amax(f2, axis=2) > 0).sum())


def test_emulator_equals_texture_map_iou_on_random_images():
    rng = np.random.default_rng(0)
    for h, w in ((5, 7), (17, 31)):
        f = rng.integers(0, 256, size=(2, h, w, 3), dtype=np.uint8) * (rng.random((2, h, w, 1)) < 0.4)
        f = f.astype(np.uint8)
        out = np.zeros((1, 4), dtype=np.int32)
        oc.emulate(pack(f[0]), pack(f[1]), h, w, [0], [0], out)
        assert out[0, 0] / (out[0, 1] + 1e-12) == texture_map_iou(f[0], f[1])


def test_case_list_covers_what_it_must():
    cases = oc.cases()
    assert {(c["h"], c["w"]) for c in cases} == set(oc.GEOMETRIES)
    assert {len(c["a_index"]) for c in cases} >= set(oc.JOB_COUNTS)
    assert len({c["name"] for c in cases}) == len(cases)
    for h, w in oc.GEOMETRIES:
        mine = [c for c in cases if (c["h"], c["w"]) == (h, w)]
        assert all(c["bev_a"].shape == (oc.STACK, h, w) and c["bev_a"].dtype == np.uint32 for c in mine)
        assert any(c["bev_b"] is c["bev_a"] for c in mine) and any(c["bad"] for c in mine)
        # the start residues of a and b, independently: every pair of images occurs in one job
        pairs = {(a, b) for c in mine if not c["bad"] for a, b in zip(c["a_index"].tolist(), c["b_index"].tolist())}
        assert len(pairs) == oc.STACK ** 2
        if (h * w) % 4:   # an odd image: its stack starts at all four residues
            assert {oc.head_pixels(k, h * w) for k in range(oc.STACK)} == {0, 1, 2, 3}
    # contents: union 0, all full, disjoint, a lone top byte that must not count, counts beyond 16 bits
    rows = np.concatenate([oc.expected(c)[0][oc.GUARD:-oc.GUARD] for c in cases if not c["bad"] and len(c["a_index"])])
    assert (rows[:, 1] == 0).any() and (rows[:, 0] == 501 * 501).any() and ((rows[:, 0] == 0) & (rows[:, 1] > 0)).any() and (rows > 65535).any()
    assert any(((c["bev_a"] & 0xFF000000) != 0).any() and ((c["bev_a"] & 0x00FFFFFF) == 0).all(axis=(1, 2)).any() for c in cases)


def test_expected_buffers_keep_their_guards_and_report_bad_jobs():
    for c in oc.cases():
        buf, raised = oc.expected(c)
        assert (buf[:oc.GUARD] == oc.SENTINEL).all() and (buf[-oc.GUARD:] == oc.SENTINEL).all()
        assert raised == c["bad"]
        body = buf[oc.GUARD:oc.GUARD + len(c["a_index"])]
        assert (body != oc.SENTINEL).all()
        ok = (c["a_index"] >= 0) & (c["a_index"] < oc.STACK) & (c["b_index"] >= 0) & (c["b_index"] < oc.STACK)
        assert (body[~ok] == -1).all() and (body[ok] >= 0).all()
        assert (body[ok, 1] == body[ok, 2] + body[ok, 3] - body[ok, 0]).all() and (body[ok, 0] <= np.minimum(body[ok, 2], body[ok, 3])).all()


@pytest.mark.parametrize("wrong", oc.WRONG_KERNELS)
def test_every_wrong_kernel_fails_a_case(wrong):
    assert len(oc.WRONG_KERNELS) >= 10
    caught = []
    for c in oc.cases():
        if c["h"] * c["w"] > 64 * 65 and wrong != "counts_16_bit":
            continue   # (the small geometries catch every other mistake; the largest is needed for counts beyond 16 bits only)
        buf, raised = oc.run_case(c, oc.emulated(wrong))
        want, want_raised = oc.expected(c)
        if not np.array_equal(buf, want) or raised != want_raised:
            caught.append(c["name"])
    assert caught, f"no case tells the wrong kernel {wrong!r} from the right one"
