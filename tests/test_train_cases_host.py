"""The shape-contract tables of tests/train_cases.py on the host (CPU): the library accepts every descriptor in them, the integer
probes meet their exactness condition, and the zero-tolerance comparators reject subtly wrong kernels emulated in float64."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

from salve_amd import _lib
from tests import train_cases as tc

ALL_CONV = tc.CONV_CASES + tc.REAL_BATCH_CASES + tc.LARGE_CASES["fp32"] + tc.LARGE_CASES["bf16"]


def _ws(query, c, pass_):
    return int(query(ctypes.byref(_lib.ConvDesc(*tc.desc_tuple(c))), pass_))


# ---------------------------------------------------------------------------------------------------- the tables themselves
def test_conv_table_holds_what_the_contract_test_needs():
    cases = tc.CONV_CASES
    assert 100 <= len(cases) <= 150 and len({tc.conv_id(c) for c in cases}) == len(cases)
    for k, s, pad in tc.FAMILIES.values():
        fam = [c for c in cases if (c.k, c.s, c.pad) == (k, s, pad)]
        assert {c.b for c in fam} >= set(tc.BATCHES), (k, s)
        assert {(c.h, c.w) for c in fam} >= set(tc.SIZES), (k, s)
        assert {c.b * c.h * c.w for c in fam} >= {127, 128, 129}, (k, s)
        assert {c.b * tc.out_size(c)[0] * tc.out_size(c)[1] for c in fam} >= set(tc.P_VALUES), (k, s)
        assert {(c.cin, c.cout) for c in fam} >= set(tc.CHANNELS), (k, s)
    stems = [c for c in cases if c.k == 7]
    assert {(c.cin, c.h, c.w) for c in stems} == {(cin, h, w) for cin in tc.STEM_CIN for h, w in tc.STEM_SIZES}
    s2 = [c for c in cases if c.s == 2 and c.k != 7]
    assert any(c.h % 2 and c.w % 2 for c in s2) and any(c.h % 2 and not c.w % 2 for c in s2) and any(not c.h % 2 and c.w % 2 for c in s2)
    assert any(tc.out_size(c)[1] < 4 for c in cases)
    assert 20 <= len(tc.RANDOM_CASES) <= 30
    assert {(c.k, c.s) for c in tc.RANDOM_CASES} == {(1, 1), (1, 2), (3, 1), (3, 2), (7, 2)}
    assert all(c.b == 256 for c in tc.REAL_BATCH_CASES) and len(tc.REAL_BATCH_CASES) == 6


def test_large_offset_cases_pass_two_to_the_31_elements_and_two_to_the_32_bytes():
    for c in tc.LARGE_CASES["fp32"]:
        assert c.b * c.h * c.w * c.cin > 2 ** 31
    for c in tc.LARGE_CASES["bf16"]:
        assert c.b * c.h * c.w * c.cin * 2 > 2 ** 32
    for prec, size in (("fp32", 4), ("bf16", 2)):
        c = tc.LARGE_CASES[prec][0]   # 1x1 / s1: the output is as large as the input
        ho, wo = tc.out_size(c)
        assert c.b * ho * wo * c.cout * size > 2 ** 32


def test_bn_table_holds_what_the_contract_test_needs():
    cases = tc.BN_CASES
    assert (tc.BN_RELU, tc.BN_ADD) == (_lib.BN_RELU, _lib.BN_ADD)
    assert {c.c for c in cases} == {8, 24, 72, 520, 4096} and {c.b * c.h * c.w for c in cases} == {2, 3, 49, 257, 12289}
    assert {(c.c, c.b * c.h * c.w) for c in cases} == {(c, r) for c in (8, 24, 72, 520, 4096) for r in (2, 3, 49, 257, 12289)}
    for c in (8, 24, 72, 520, 4096):
        assert {k.flags for k in cases if k.c == c} == {0, 1, 2, 3}, c
    for r in (2, 3, 49, 257, 12289):
        assert {k.flags for k in cases if k.b * k.h * k.w == r} == {0, 1, 2, 3}, r
    assert {(k.b, k.c, k.h, k.w) for k in tc.BN_REAL_BATCH_CASES} == {(256, 2048, 7, 7), (256, 64, 56, 56)}
    assert {(k.c, k.b * k.h * k.w) for k in tc.BN_DETERMINISM_CASES} == {(520, 12289), (8, 3)}


# ---------------------------------------------------------------------------------------------------- the library's contract
def test_workspace_queries_accept_every_convolution_descriptor():
    lib = _lib.load()
    for query in (lib.salve_conv_f32_workspace_bytes, lib.salve_conv_bf16_workspace_bytes):
        for c in ALL_CONV:
            assert _ws(query, c, _lib.CONV_FWD) > 0 and _ws(query, c, _lib.CONV_WGRAD) >= 256, tc.conv_id(c)
            assert (_ws(query, c, _lib.CONV_DGRAD) > 0) == (c.k != 7), tc.conv_id(c)


def test_wgrad_runs_with_one_split_and_with_several_in_both_precisions():
    """The workspace query is the public view of the wgrad split: 256 bytes = one split (dW written directly), more = partial slabs."""
    lib = _lib.load()
    for query in (lib.salve_conv_f32_workspace_bytes, lib.salve_conv_bf16_workspace_bytes):
        sizes = [_ws(query, c, _lib.CONV_WGRAD) for c in tc.CONV_CASES]
        assert sizes.count(256) >= 10 and sum(s > 256 for s in sizes) >= 10
        assert all(_ws(query, c, _lib.CONV_WGRAD) > 256 for c in tc.REAL_BATCH_CASES + tc.LARGE_CASES["fp32"])


def test_workspace_query_accepts_every_batchnorm_descriptor():
    lib = _lib.load()
    for c in tc.BN_CASES + tc.BN_REAL_BATCH_CASES + tc.BN_DETERMINISM_CASES:
        for pass_ in (_lib.BN_FWD, _lib.BN_BWD):
            assert int(lib.salve_bn_workspace_bytes(ctypes.byref(_lib.BnDesc(c.b * c.h * c.w, c.c, c.flags, 1e-5, 0.1)), pass_)) > 0, tc.bn_id(c)


# ---------------------------------------------------------------------------------------------------- the exactness condition
@pytest.mark.parametrize("c", ALL_CONV, ids=tc.conv_id)
def test_probe_meets_the_exactness_condition(c):
    x, w, dy = tc.probe_operands(c)
    assert x.shape[0] == (c.b if c.b <= 8 else tc.D_SAMPLES)
    assert set(x.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert set(dy.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    sums = tc.abs_term_sums(c, x, w, dy)
    print(tc.conv_id(c), sums)
    assert all(v <= tc.EXACT_LIMIT for v in sums.values()), sums
    if c.b > 8:
        idx = tc.sample_index(c)
        assert idx.shape == (c.b,) and set(idx.tolist()) == set(range(tc.D_SAMPLES))


# ---------------------------------------------------------------------------------------------------- wrong kernels, emulated
def _tile_unwritten(t, tile=128):
    """The last `tile`-pixel tile of the NHWC pixel list left unwritten (zeros)."""
    n = t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).clone()
    n[(n.shape[0] - 1) // tile * tile:] = 0
    return n.reshape(t.shape[0], t.shape[2], t.shape[3], t.shape[1]).permute(0, 3, 1, 2)


def _hw_swapped(t):
    """Pixel (y, x) stored where a kernel that takes the image for W x H would put it."""
    return t.transpose(2, 3).reshape(t.shape)


def _chunk_shifted(t):
    """Channels 8..15 read from (written as) channels 16..23; a stem's 6 / 12 / 18 channels: chunk 0 from chunk 1 of the padded input."""
    if t.shape[1] >= 24:
        t = t.clone()
        t[:, 8:16] = t[:, 16:24]
        return t
    padded = F.pad(t, (0, 0, 0, 0, 0, 16 - t.shape[1]))
    return torch.cat([padded[:, 8:16], padded[:, 8:]], 1)[:, :t.shape[1]]


def _last_pixel_dropped(t):
    t = t.clone()
    t[-1, :, -1, -1] = 0
    return t


def _shift_one(t):
    """Every pixel moved by one row and one column (a parity test off by one sends each tap to the neighbouring pixel)."""
    return F.pad(t, (1, 0, 1, 0))[:, :, :t.shape[2], :t.shape[3]]


def wrong_outputs(c, x, w, dy):
    """{pass: {emulated bug: output}} for one case, each a few lines of torch on the float64 reference path."""
    conv = lambda x_, w_: F.conv2d(x_, w_, stride=c.s, padding=c.pad)   # noqa: E731
    dgrad = lambda w_, dy_: torch.nn.grad.conv2d_input(x.shape, w_, dy_, stride=c.s, padding=c.pad)   # noqa: E731
    wgrad = lambda x_, dy_: torch.nn.grad.conv2d_weight(x_, w.shape, dy_, stride=c.s, padding=c.pad)   # noqa: E731
    fwd, dg, wg = conv(x, w), (None if c.k == 7 else dgrad(w, dy)), wgrad(x, dy)
    bad = {"fwd": {"H and W swapped": _hw_swapped(fwd), "last M tile unwritten": _tile_unwritten(fwd),
                   "sample b reads b+1": conv(x.roll(-1, 0), w), "input chunk shifted": conv(_chunk_shifted(x), w),
                   "output chunk shifted": _chunk_shifted(fwd)},
           "wgrad": {"H and W swapped": wgrad(_hw_swapped(x), dy), "last pixel of P dropped": wgrad(x, _last_pixel_dropped(dy)),
                     "x[b] paired with dy[b+1]": wgrad(x, dy.roll(-1, 0)), "dy chunk shifted": wgrad(x, _chunk_shifted(dy)),
                     "x chunk shifted": wgrad(_chunk_shifted(x), dy)}}
    if c.k > 1:
        bad["fwd"]["ky and kx swapped"] = conv(x, w.transpose(2, 3))
        bad["wgrad"]["ky and kx swapped"] = wg.transpose(2, 3)
    if dg is not None:
        bad["dgrad"] = {"H and W swapped": _hw_swapped(dg), "last M tile unwritten": _tile_unwritten(dg),
                        "sample b reads b+1": dgrad(w, dy.roll(-1, 0)), "dy chunk shifted": dgrad(w, _chunk_shifted(dy)),
                        "output chunk shifted": _chunk_shifted(dg)}
        if c.k > 1:
            bad["dgrad"]["ky and kx swapped"] = dgrad(w.transpose(2, 3), dy)
            bad["dgrad"]["taps not rotated"] = dgrad(w.flip(2, 3), dy)
        if c.s == 2:
            bad["dgrad"]["parity test off by one"] = _shift_one(dg)
    return {"fwd": fwd, "dgrad": dg, "wgrad": wg}, bad


@pytest.mark.parametrize("family", list(tc.REPRESENTATIVE))
def test_comparators_reject_emulated_wrong_kernels(family):
    c = tc.REPRESENTATIVE[family]
    p = tc.build_probe(c)
    ref, bad = wrong_outputs(c, p["x"], p["w"], p["dy"])
    assert torch.equal(ref["fwd"], p["fwd"]) and torch.equal(ref["wgrad"], p["wgrad"])
    assert tc.exact_f32(ref["fwd"].float(), p["fwd"]) and tc.exact_bf16(ref["fwd"].to(torch.bfloat16), p["fwd"])
    assert tc.exact_f32(ref["wgrad"].float(), p["wgrad"])
    expected = {"fwd": 5 + (c.k > 1), "wgrad": 5 + (c.k > 1)}
    if c.k != 7:
        assert tc.exact_f32(ref["dgrad"].float(), p["dgrad"]) and tc.exact_bf16(ref["dgrad"].to(torch.bfloat16), p["dgrad"])
        expected["dgrad"] = 5 + 2 * (c.k > 1) + (c.s == 2)
    assert {k: len(v) for k, v in bad.items()} == expected
    for pass_, outs in bad.items():
        for bug, out in outs.items():
            n_diff = int((out != ref[pass_]).sum())
            print(f"{tc.conv_id(c)} {pass_} {bug}: {n_diff} of {out.numel()} elements differ")
            assert n_diff > 0, (pass_, bug)                                  # the probe has weight on this bug
            assert not tc.exact_f32(out.float(), p[pass_]), (pass_, bug)     # ... and the fp32 comparator sees it
            if pass_ != "wgrad":                                             # ... and so does the bf16 one, after its rounding
                assert not tc.exact_bf16(out.to(torch.bfloat16), p[pass_]), (pass_, bug)


def test_replicated_comparator_rejects_wrong_samples_and_wrong_pairs():
    c = tc.REPLICATED_REPRESENTATIVE
    p = tc.build_probe(c)
    idx = p["idx"]
    assert p["x"].shape[0] == tc.D_SAMPLES and idx.shape == (c.b,)
    xb, dyb = tc.replicate(p["x"], idx), tc.replicate(p["dy"], idx)
    assert xb.is_contiguous(memory_format=torch.channels_last) and all(torch.equal(xb[b], p["x"][idx[b]]) for b in range(c.b))
    ref, bad = wrong_outputs(c, xb, p["w"], dyb)   # the whole batch in float64: small enough here
    assert torch.equal(ref["wgrad"], p["wgrad"])   # sum_d count_d * dW_d is the batch's dW
    for pass_, cmp, cast in (("fwd", tc.exact_f32, torch.float32), ("dgrad", tc.exact_f32, torch.float32),
                             ("fwd", tc.exact_bf16, torch.bfloat16), ("dgrad", tc.exact_bf16, torch.bfloat16)):
        assert tc.exact_replicated(ref[pass_].to(cast), p[pass_], idx, cmp, chunk=5)
        assert not tc.exact_replicated(ref[pass_].to(cast)[:-1], p[pass_], idx, cmp, chunk=5)
        for bug, out in bad[pass_].items():
            assert not tc.exact_replicated(out.to(cast), p[pass_], idx, cmp, chunk=5), (pass_, bug)
    for bug, out in bad["wgrad"].items():
        assert not tc.exact_f32(out.float(), p["wgrad"]), bug


def test_bf16_comparator_is_one_rounding_of_the_exact_sum():
    ref = torch.tensor([257.0, 258.0, 259.0, -1027.0, 2.0 ** 22 - 1])   # ties go to even, 259 up to 260
    assert tc.exact_bf16(torch.tensor([256.0, 258.0, 260.0, -1028.0, 2.0 ** 22]).to(torch.bfloat16), ref.double())
    assert not tc.exact_bf16(torch.tensor([258.0, 258.0, 260.0, -1028.0, 2.0 ** 22]).to(torch.bfloat16), ref.double())
    assert not tc.exact_f32(torch.tensor([1.0]), torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
