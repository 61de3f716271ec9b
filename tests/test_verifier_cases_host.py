"""The probes, the emulator and the mutants of tests/verifier_cases.py, checked on the host: the emulator without its rounding step is
torch's float64 operation, every case meets the exactness condition, every mutant is seen by every case of the families it applies
to, the multi-op programs are alive, and the emulator reads the op format that hip_resnet.build_program really packs."""

from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import verifier_cases as vc  # noqa: E402
from _helpers import randomise_bn  # noqa: E402
from oracle import resnet_oracle as ro  # noqa: E402
from salve_amd import _lib  # noqa: E402
from salve_amd.models import hip_resnet  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402

_CACHE = {}


def true_run(key, make):
    """check_exact's emulation of a program, computed once per case and shared (never modified)."""
    if key not in _CACHE:
        prog = make()
        _CACHE[key] = (prog, vc.check_exact(prog))
    return _CACHE[key]


def differs(a, b, read):
    return any(not torch.equal(a[0][i], b[0][i]) for i in read)


def test_flag_values_are_the_bindings():
    assert (vc.IGEMM_ONLY, vc.CONV8_WHEREVER, vc.NO_STEM_FUSE, vc.NO_BLOCK_FUSE, vc.NO_CHAIN, vc.NO_NEXT_FUSE) == (
        _lib.RESNET_CONV_IGEMM_ONLY, _lib.RESNET_CONV8_WHEREVER, _lib.RESNET_NO_STEM_FUSE, _lib.RESNET_NO_BLOCK_FUSE, _lib.RESNET_NO_CHAIN, _lib.RESNET_NO_NEXT_FUSE)


def test_round_fp16_is_torchs_conversion_and_ties_go_to_even():
    g = torch.Generator().manual_seed(0)
    v = torch.randn(20000, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-8, 5, (20000,), generator=g).double()
    v = torch.cat([v, v.float().double(), torch.tensor([0.0, 65504.0, -65504.0, 65519.0, 1e9, -1e9, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25])])
    assert torch.equal(vc.round_fp16(v.float().double()), v.float().clamp(-65504, 65504).to(torch.float16).double())
    ties = torch.tensor([32 + 1 / 64, 32 + 3 / 64, -(32 + 1 / 64), -(32 + 3 / 64), 2049.0, 2051.0], dtype=torch.float64)
    assert vc.round_fp16(ties).tolist() == [32.0, 32.0625, -32.0, -32.0625, 2048.0, 2052.0]
    assert vc.round_fp16(ties, "away").tolist() == [32.03125, 32.0625, -32.03125, -32.0625, 2050.0, 2052.0]


# ------------------------------------------------------------------------------------------------ the emulator is the float64 operation
@pytest.mark.parametrize("c", [fam[7] for fam in vc.CONV_CASES.values()] + [fam[-1] for fam in vc.CONV_CASES.values()] + vc.STEM_CASES[-3:] +
                         [vc.CONV_CASES["k3s1"][-2]], ids=vc.case_id)
def test_unrounded_convolution_is_conv2d(c):
    """The emulator's reading of the packed weights (k table, padded kw and channels, group-major stems) against F.conv2d on the
    unpacked tensors, random operands, residual and ReLU as the case has them."""
    g = torch.Generator().manual_seed(3)
    cp = hip_resnet.pad_channels(c.cin)
    w = torch.randn(c.cout, c.cin, c.k, c.k, generator=g).to(torch.float16)
    b = torch.randn(c.cout, generator=g)
    x = torch.zeros(c.b, c.h, c.w, cp, dtype=torch.float64)
    x[..., :c.cin] = torch.randn(c.b, c.h, c.w, c.cin, generator=g, dtype=torch.float64)
    ho, wo = vc.out_size(c)
    res = torch.randn(c.b, ho, wo, c.cout, generator=g, dtype=torch.float64) if c.res else None
    bld = hip_resnet._Builder()
    bld.conv(w.float(), b, hip_resnet.NET_INPUT, 0, 1 if c.res else hip_resnet.NO_BUF, c.h, c.w, c.s, c.pad, bool(c.relu), c.kw_pad)
    em = vc.Emulator(*vc.pack(bld), rounding=None)
    got = em.run_op(0, {hip_resnet.NET_INPUT: x, 1: res})
    ref = F.conv2d(x[..., :c.cin].permute(0, 3, 1, 2), w.double(), b.double(), c.s, c.pad).permute(0, 2, 3, 1)
    ref = ref + res if c.res else ref
    ref = ref.relu() if c.relu else ref
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("c", [vc.SRC2_CASES[1], vc.SRC2_CASES[4]], ids=vc.case_id)
def test_unrounded_second_source_is_two_convolutions(c):
    prog = vc.conv_program(c, random=True)
    em = vc.Emulator(*vc.pack(prog.bld), rounding=None)
    bufs, _, _ = em.run(prog.x)
    cin2, s2 = c.src2
    rows = em.weights[int(em.ops[1]["w_off"]):].view(np.float16).astype(np.float64).reshape(c.cout, c.cin + cin2)
    bias = torch.from_numpy(em.params[int(em.ops[1]["b_off"]):].astype(np.float64))
    t2, x = bufs[0].permute(0, 3, 1, 2), prog.x.permute(0, 3, 1, 2)
    ref = (F.conv2d(t2, torch.from_numpy(rows[:, :c.cin].copy())[:, :, None, None]) +
           F.conv2d(x, torch.from_numpy(rows[:, c.cin:].copy())[:, :, None, None], stride=s2) + bias[None, :, None, None]).relu().permute(0, 2, 3, 1)
    assert float((bufs[1] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("c", vc.MAXPOOL_CASES[::3], ids=vc.pool_id)
def test_emulated_maxpool_is_max_pool2d(c):
    prog = vc.maxpool_program(c)
    bufs, _, _ = vc.emulate(prog)
    assert torch.equal(bufs[0], F.max_pool2d(prog.x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))


@pytest.mark.parametrize("c", vc.FC_CASES[::4], ids=vc.pool_id)
def test_emulated_classifier_is_avg_pool_and_linear(c):
    prog = vc.fc_program(c)
    em = vc.Emulator(*vc.pack(prog.bld))
    _, logits, _ = em.run(prog.x)
    w = torch.from_numpy(em.params[:c.ncls * c.c].astype(np.float64).reshape(c.ncls, c.c))
    b = torch.from_numpy(em.params[c.ncls * c.c:].astype(np.float64))
    ref = F.linear(F.adaptive_avg_pool2d(prog.x.permute(0, 3, 1, 2), 1).flatten(1), w, b)
    assert float((logits - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ exactness and mutants, every case
@pytest.mark.parametrize("c", vc.ALL_CONV_CASES, ids=vc.case_id)
def test_conv_probe_is_exact_and_sees_every_mutant(c):
    prog, true = true_run(("conv", c), lambda: vc.conv_program(c))
    for i, (h, w, ch) in prog.read.items():
        assert tuple(true[0][i].shape) == (c.b, h, w, ch)
    ho, wo = vc.out_size(c)
    for m in vc.MUTANTS:
        if not vc.mutant_applies(m, c):
            continue
        tiles = [128] + ([256] if c in vc.CONV8_CASES and c.b * ho * wo >= 256 else []) if m == "m_tile_edge_row" else [128]
        for tile in tiles:
            assert differs(true, vc.emulate(prog, mutant=m, m_tile=tile), prog.read), f"{vc.case_id(c)} cannot see {m} (tile {tile})"


def test_every_conv_mutant_has_cases_in_every_family_it_belongs_to():
    families = dict(vc.CONV_CASES, stem=vc.STEM_CASES, src2=vc.SRC2_CASES, conv8=vc.CONV8_CASES)
    want = {"taps_transposed": {"k3s1", "k3s2", "stem", "conv8"}, "padding_is_a_pixel": {"k3s1", "k3s2", "stem", "conv8"},
            "m_tile_edge_row": set(families) - {"stem"}, "stem_groups_swapped": {"stem"}, "residual_after_relu": {"k1s1", "k3s1", "k3s2", "conv8"},
            "round_half_away": set(families), "src2_stride_1": {"src2"}}
    for m, fams in want.items():
        for f in fams:
            assert any(vc.mutant_applies(m, c) for c in families[f]), (m, f)
    assert {c.cin for c in vc.STEM_CASES if vc.mutant_applies("stem_groups_swapped", c)} == {12, 18}
    ms = sorted(c.b * vc.out_size(c)[0] * vc.out_size(c)[1] for fam in vc.CONV_CASES.values() for c in fam)
    assert {127, 128, 129} <= set(ms)
    assert {255, 256, 257} <= {c.b * vc.out_size(c)[0] * vc.out_size(c)[1] for c in vc.CONV8_CASES}


@pytest.mark.parametrize("c", vc.MAXPOOL_CASES, ids=vc.pool_id)
def test_maxpool_probe_sees_zero_padding(c):
    prog, true = true_run(("pool", c), lambda: vc.maxpool_program(c))
    out, mut = true[0][0], vc.emulate(prog, mutant="maxpool_zero_padding")[0][0]
    assert (out < 0).any() and not torch.equal(out, mut)
    edge = torch.zeros(out.shape[1:3], dtype=torch.bool)
    edge[0], edge[:, 0] = True, True
    if c.h % 2:
        edge[-1] = True     # (an even size: the last window ends at the last pixel and does not touch the padding)
    if c.w % 2:
        edge[:, -1] = True
    assert (out != mut).any(-1).any(0)[edge].all(), "every window that touches the padding is all negative"


@pytest.mark.parametrize("c", vc.FC_CASES, ids=vc.pool_id)
def test_classifier_probe_is_exact_and_sees_the_wrong_divisor(c):
    prog = vc.fc_program(c)
    if vc.fc_exact(c):
        prog, true = true_run(("fc", c), lambda: prog)
        logits = true[1]
        assert torch.equal(logits, logits.float().double())
    else:
        logits = vc.emulate(prog)[1]
    assert not torch.equal(logits, vc.emulate(prog, mutant="avgpool_wrong_hw")[1])
    assert tuple(logits.shape) == (c.b, c.ncls)


def test_the_pool_tables_cover_the_issue():
    assert {c.c for c in vc.MAXPOOL_CASES} == {8, 64, 72} and {(1, 1), (13, 29)} <= {(c.h, c.w) for c in vc.MAXPOOL_CASES}
    assert {c.h * c.w for c in vc.FC_CASES} == {1, 4, 16, 64, 49, 35}
    assert {c.c for c in vc.FC_CASES} == {8, 512, 2048, 2056, 4096}
    for hw in (1, 4, 16, 64, 49, 35):
        assert {c.ncls for c in vc.FC_CASES if c.h * c.w == hw} == {1, 2, 3, 8}
    assert {c.ncls for c in vc.FC_CASES if c.c > 2048} == {1, 2, 3, 8}


# ------------------------------------------------------------------------------------------------ programs
def _alive(prog, true):
    for i in prog.read:
        share = float((true[0][i] != 0).double().mean())
        assert share > 0.2, f"{prog.name}: buffer {i} is {share:.0%} non-zero"


@pytest.mark.parametrize("h,w", vc.BLOCK_SIZES)
@pytest.mark.parametrize("b", vc.BLOCK_BATCHES)
def test_block_program_is_exact_and_alive(h, w, b):
    prog, true = true_run(("block", h, w, b), lambda: vc.block_program(h, w, b))
    _alive(prog, true)
    for m in ("taps_transposed", "padding_is_a_pixel", "round_half_away", "src2_stride_1"):
        assert differs(true, vc.emulate(prog, mutant=m), prog.read), (prog.name, m)


@pytest.mark.parametrize("mid,midn,b,h,w", vc.CHAIN_CASES)
def test_chain_program_is_exact_and_alive(mid, midn, b, h, w):
    prog, true = true_run(("chain", mid, midn, b, h, w), lambda: vc.chain_program(mid, midn, b, h, w))
    _alive(prog, true)
    for m in ("residual_after_relu", "round_half_away") + (("m_tile_edge_row",) if b * h * w >= 128 else ()):
        assert differs(true, vc.emulate(prog, mutant=m), prog.read), (prog.name, m)


@pytest.mark.parametrize("cin,h,b", vc.STEM_POOL_CASES)
def test_stem_program_is_exact_and_sees_its_mutants(cin, h, b):
    prog, true = true_run(("stem", cin, h, b), lambda: vc.stem_program(cin, h, b))
    # (not maxpool_zero_padding: the pool reads ReLU outputs, for which a zero is as good as minus infinity -- MAXPOOL_CASES see it)
    for m in ("taps_transposed", "padding_is_a_pixel", "round_half_away") + (("stem_groups_swapped",) if cin > 6 else ()):
        mut = vc.emulate(prog, mutant=m)
        assert not torch.equal(true[0][1], mut[0][1]), f"{prog.name}: the pooled tensor cannot see {m}"


def test_chain_and_block_tables_cover_the_issue():
    assert set(vc.NEW_WIDTH_BLOCKS) <= set(vc.BLOCK_SIZES) and {(24, 40), (16, 56), (56, 56), (8, 16)} <= set(vc.BLOCK_SIZES)
    ms = {b * h * w for mid, midn, b, h, w in vc.CHAIN_CASES if (mid, midn) == (128, 256)}
    assert {127, 128, 129, 255, 256, 257} <= ms
    assert any(vc.chain_program(*c).even is not None for c in vc.CHAIN_CASES[:3])
    assert {(cin, h) for cin, h, _ in vc.STEM_POOL_CASES} == {(c, h) for c in (6, 12, 18) for h in (16, 32, 48)}


# ------------------------------------------------------------------------------------------------ the real op format
def test_emulator_reads_the_program_of_a_resnet50_state_dict():
    """hip_resnet.build_program's arrays for ResNet-50 (12 input channels: the group-major stem) on a 2 x 32 x 32 input: the emulator
    with the kernels' rounding points gives the oracle's logits within the project's contract, 1e-3 x max(1, |logit|), and without
    them within the fp16 rounding of the weights alone."""
    torch.manual_seed(3)
    model = EarlyFusionCEResnet(50, False, 2, SimpleNamespace(modalities=["ceiling_rgb_texture", "floor_rgb_texture"]))
    randomise_bn(model, seed=3)
    model.eval()
    sd = model.state_dict()
    ops, wbits, params, ktab, cin_p = hip_resnet.build_program(sd, 50, in_hw=(32, 32))
    assert cin_p == 16 and len(ops) == 1 + 1 + 16 * 3 + 1
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(2, 3, 32, 32, generator=g) for _ in range(4)]
    x = hip_resnet.nchw_to_input(xs, cin_p).double()
    with torch.no_grad():
        ref = ro.forward(sd, 50, xs).double()
    scale = max(1.0, float(ref.abs().max()))
    _, logits, stores = vc.Emulator(ops, wbits, params, ktab).run(x)
    assert len(stores) == len(ops) and tuple(logits.shape) == (2, 2)
    assert float((logits - ref).abs().max()) <= 1e-3 * scale
    _, plain, _ = vc.Emulator(ops, wbits, params, ktab, rounding=None).run(x)
    assert float((plain - ref).abs().max()) <= 1e-3 * scale
    assert not torch.equal(plain, logits), "the rounding points must do something"
