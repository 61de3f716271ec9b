"""The fp16 verifier's kernels against arithmetic done outside the library (tests/verifier_cases.py): integer probes whose fp32 sums are
exact in any order, emulated in float64 with the kernels' rounding points and compared bit for bit, over the op contract that
salve_resnet_create accepts -- every convolution family at odd, non-square and tile-edge shapes, the second-source form, the 8-phase
kernel, the fused stem, the fused 56 x 56 block at every width residue, the expand + chain kernels, the max-pool and the classifier on
their own.  Both sides of every bit-identity test of test_gpu_verifier.py are anchored: each fused program runs under flags 0 and with
its fusion switched off.  Every program goes through salve_resnet_create(flags) / salve_resnet_forward with the workspace pre-filled
with fp16 NaNs and a status word that must stay 0."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import verifier_cases as vc  # noqa: E402
from salve_amd import _lib  # noqa: E402
from salve_amd.models.hip_resnet import NET_INPUT, OP_AVGPOOL_FC  # noqa: E402

DEV = "cuda:0"
_REF = {}


def reference(key, make):
    """(program, its emulation): computed once per case, shared between the flag settings, never modified."""
    if key not in _REF:
        prog = make()
        _REF[key] = (prog, vc.emulate(prog))
    return _REF[key]


def run_program(prog, flags, expect_status=0):
    """The program through salve_resnet_create(flags) / salve_resnet_forward -> ({buffer: int16 bits [B, H, W, C]}, fp32 logits or None)."""
    lib = _lib.load()
    ops, wb, pr, kt = vc.pack(prog.bld)
    x = vc.fp16_bits(prog.x).contiguous()
    B, Cp = int(x.shape[0]), int(x.shape[3])
    h = lib.salve_resnet_create(0, Cp, ops.ctypes.data_as(ctypes.c_void_p), len(ops), wb.ctypes.data_as(ctypes.c_void_p), wb.nbytes,
                                pr.ctypes.data_as(ctypes.c_void_p), pr.nbytes, kt.ctypes.data_as(ctypes.c_void_p), kt.size, int(flags))
    assert h, lib.salve_last_error()
    h = ctypes.c_void_p(h)
    try:
        need = lib.salve_resnet_workspace_bytes(h, B)
        stored = [o for o in ops if int(o["op"]) != OP_AVGPOOL_FC]
        n_bufs = max((int(o["out_buf"]) for o in stored), default=-1) + 1
        ncls = max([int(o["Cout"]) for o in ops if int(o["op"]) == OP_AVGPOOL_FC], default=2)
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        base_off = (-ws.data_ptr()) % 256
        view = ws[base_off:base_off + (need - 256)].view(torch.int16)
        view.fill_(vc.NAN_BITS)                  # a pixel a kernel fails to write shows up
        per_buf = view.numel() // max(n_bufs, 1)
        logits = torch.full((B, ncls), float("nan"), dtype=torch.float32, device=DEV)
        xd = x.to(DEV)
        word = torch.zeros(1, dtype=torch.int32, device=DEV)
        st = lib.salve_resnet_forward(h, ctypes.c_void_p(xd.data_ptr()), B, ctypes.c_void_p(logits.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                      ws.numel(), ctypes.c_void_p(word.data_ptr()), None)
        torch.cuda.synchronize()
        assert st == 0, lib.salve_last_error()
        assert int(word.item()) == expect_status, f"status word {int(word.item())}"
        out = {i: view[i * per_buf: i * per_buf + B * H * W * C].clone().cpu().reshape(B, H, W, C) for i, (H, W, C) in prog.read.items()}
        return out, (logits.cpu() if any(int(o["op"]) == OP_AVGPOOL_FC for o in ops) else None)
    finally:
        lib.salve_resnet_destroy(h)


def assert_exact(prog, ref, flags, even=False, skip=()):
    """Every readable buffer bit for bit against the emulation; even: the program's `even` buffer holds its even pixels only."""
    got, _ = run_program(prog, flags)
    reports = []
    for i in prog.read:
        if i in skip:
            continue
        g_, r_ = got[i], vc.fp16_bits(ref[0][i])
        if even and i == prog.even:
            assert (g_[:, 1::2] == vc.NAN_BITS).all() and (g_[:, :, 1::2] == vc.NAN_BITS).all(), f"{prog.name}: odd pixels of buffer {i} were meant to stay unwritten"
            g_, r_ = g_[:, ::2, ::2], r_[:, ::2, ::2]
        reports.append(vc.diff_report(g_, r_, f"{prog.name}, flags {flags}, buffer {i}"))
    bad = [r for r in reports if r]
    if bad:
        print("\n".join(bad))
    assert not bad, bad[0]


# ------------------------------------------------------------------------------------------------ probes, exact: the fused programs
@pytest.mark.parametrize("h,w", vc.BLOCK_SIZES)
@pytest.mark.parametrize("b", vc.BLOCK_BATCHES)
def test_fused_block_program_matches_the_emulator_bit_for_bit(h, w, b):
    """bottleneck_kernel PROJ and NEXT (flags 0), plain (NO_NEXT_FUSE: Y stored whole, the next 1x1 a launch of its own) and the
    three-kernel path (NO_BLOCK_FUSE) against the float64 emulation, the five readable tensors each.  W = 8: no upright tile, every tile transposed; 20 and 13: a partly empty last tile column; 40 and 56: the
    transposed strip; square sizes store Y's even pixels only."""
    prog, ref = reference(("block", h, w, b), lambda: vc.block_program(h, w, b))
    for flags in (0, vc.NO_STEM_FUSE, vc.NO_BLOCK_FUSE, vc.NO_CHAIN, vc.NO_NEXT_FUSE):
        assert_exact(prog, ref, flags, even=prog.even is not None and not flags & (vc.NO_BLOCK_FUSE | vc.NO_NEXT_FUSE))


@pytest.mark.parametrize("cin,h,b", vc.STEM_POOL_CASES)
def test_stem_program_matches_the_emulator_bit_for_bit(cin, h, b):
    """stem_pool_kernel<1|2|3> at H = 16, 32, 48 (flags 0: the un-pooled tensor is never stored) and the implicit-GEMM stem + maxpool_kernel."""
    prog, ref = reference(("stem", cin, h, b), lambda: vc.stem_program(cin, h, b))
    for flags in (0, vc.NO_BLOCK_FUSE, vc.NO_CHAIN):
        assert_exact(prog, ref, flags, skip=(0,))
    assert_exact(prog, ref, vc.NO_STEM_FUSE)


@pytest.mark.parametrize("mid,midn,b,h,w", vc.CHAIN_CASES)
def test_chain_program_matches_the_emulator_bit_for_bit(mid, midn, b, h, w):
    """expand_chain_kernel chained ((128, 256): Y's even pixels only at square even sizes) and expand-only (no chained form for (256, 128),
    (128, 64)) under flags 0, conv_igemm_kernel's residual epilogue under NO_CHAIN."""
    prog, ref = reference(("chain", mid, midn, b, h, w), lambda: vc.chain_program(mid, midn, b, h, w))
    for flags in (0, vc.NO_STEM_FUSE, vc.NO_BLOCK_FUSE, vc.NO_CHAIN):
        assert_exact(prog, ref, flags, even=prog.even is not None and not flags & vc.NO_CHAIN)


# ------------------------------------------------------------------------------------------------ probes, exact: single ops
@pytest.mark.parametrize("c", vc.ALL_CONV_CASES, ids=vc.case_id)
def test_convolution_probe_matches_the_emulator_bit_for_bit(c):
    """conv_igemm_kernel in its six instantiations (BN 64 / 128, point-wise, gather, second source); the conv8 cases again on
    conv8_kernel.  A residual comes from a producer op; a second source is the network input."""
    prog, ref = reference(("conv", c), lambda: vc.conv_program(c))
    assert_exact(prog, ref, vc.IGEMM_ONLY)
    if c in vc.CONV8_CASES:
        assert_exact(prog, ref, vc.CONV8_WHEREVER)


@pytest.mark.parametrize("c", vc.MAXPOOL_CASES, ids=vc.pool_id)
def test_maxpool_matches_the_emulator_bit_for_bit(c):
    prog, ref = reference(("pool", c), lambda: vc.maxpool_program(c))
    assert_exact(prog, ref, 0)


@pytest.mark.parametrize("c", vc.FC_CASES, ids=vc.pool_id)
def test_classifier_matches_float64(c):
    """1 / HW a power of two: the probes keep every fp32 sum exact and the logits equal the float64 ones.  Otherwise within 10 x the error
    of torch's fp32 CPU result on the same inputs against float64, floored at one fp32 ulp of the largest logit."""
    prog, ref = reference(("fc", c), lambda: vc.fc_program(c))
    _, got = run_program(prog, 0)
    want = ref[1]
    assert tuple(got.shape) == (c.b, c.ncls)
    err = float((got.double() - want).abs().max())
    if vc.fc_exact(c):
        print(f"{prog.name}: max |logit| {float(want.abs().max())}, error {err}")
        assert torch.equal(got.double(), want), (got, want)
        return
    ops, _, params, _ = vc.pack(prog.bld)
    w = torch.from_numpy(params[:c.ncls * c.c].reshape(c.ncls, c.c))
    b = torch.from_numpy(params[c.ncls * c.c: c.ncls * c.c + c.ncls])
    fp32 = F.linear(F.adaptive_avg_pool2d(prog.x.float().permute(0, 3, 1, 2), 1).flatten(1), w, b)
    err32 = float((fp32.double() - want).abs().max())
    bound = max(10.0 * err32, float(np.spacing(np.float32(float(want.abs().max())))))
    print(f"{prog.name}: max |logit| {float(want.abs().max()):.3f}, error {err:.3e}, torch fp32 CPU {err32:.3e}, bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------------------------------------ random operands
@pytest.mark.parametrize("c", vc.RANDOM_CASES, ids=vc.case_id)
def test_random_operands_within_one_rounding_of_float64(c):
    """Normal operands (fp16): every op of the program against float64 ON THE BUFFERS IT READ, |got - r| <= 2^-11 |r| + 2^-20 A + 2^-25
    elementwise -- half an fp16 ulp, the fp32 accumulation term on the same op over absolute operands, the fp16 subnormal spacing."""
    prog = vc.conv_program(c, random=True)
    flags = [vc.IGEMM_ONLY] + ([vc.CONV8_WHEREVER] if c in vc.CONV8_CASES else [])
    arrays = vc.pack(prog.bld)
    plain, terms = vc.Emulator(*arrays, rounding=None), vc.Emulator(*arrays, rounding=None, absolute=True)
    for f in flags:
        got, _ = run_program(prog, f)
        bufs = {NET_INPUT: prog.x, **{i: g_.view(torch.float16).double() for i, g_ in got.items()}}
        assert all(torch.isfinite(t).all() for t in bufs.values())
        for i, o in enumerate(arrays[0]):
            r, a = plain.run_op(i, bufs), terms.run_op(i, {k: v.abs() for k, v in bufs.items()})
            err, bound = (bufs[int(o["out_buf"])] - r).abs(), vc.rounded_bound(r, a)
            worst = float((err / bound).max())
            print(f"{prog.name}, flags {f}, op {i}: max |r| {float(r.abs().max()):.3f}, max error {float(err.max()):.3e}, worst error / bound {worst:.3f}")
            bad = (err > bound).nonzero()
            assert len(bad) == 0, f"{prog.name}, op {i}: {len(bad)} values beyond the bound, first at {bad[:3].tolist()}"


# ------------------------------------------------------------------------------------------------ non-finite inputs stay local
def test_non_finite_inputs_stay_local():
    """An fp16 infinity at two interior pixels of a 3x3 / stride 2 gather without ReLU.  The engine stores no infinity by contract
    (include/salve_hip.h: the store saturates at +-65504 and raises SALVE_STATUS_FP16_RANGE;
    test_convolution_without_relu_saturates_and_reports_both_signs), so `isfinite` of its output is true everywhere and a non-finite sum
    reads as a stored +-65504.  The locality asserted, element for element: the outputs that store +-65504 are exactly the outputs whose
    float64 convolution is not finite, every other output keeps the bits of the run without the infinities, and the status word reports
    the range."""
    c, pixels = vc.NON_FINITE_CASE
    clean = vc.conv_program(c, random=True)
    x = clean.x.clone()
    for b, y, x_ in pixels:
        x[b, y, x_, 0] = float("inf")   # one channel: every sum that meets it is an infinity, not inf - inf
    prog = clean._replace(x=x)
    want = ~torch.isfinite(vc.emulate(prog, rounding=None)[0][0])
    base, _ = run_program(clean, vc.IGEMM_ONLY)
    got, _ = run_program(prog, vc.IGEMM_ONLY, expect_status=_lib.STATUS_FP16_RANGE)
    vals = got[0].view(torch.float16).double()
    assert torch.isfinite(vals).all()
    hit = vals.abs() == vc.FP16_MAX
    extra, missing = (hit & ~want).nonzero(), (~hit & want).nonzero()
    print(f"{int(want.sum())} outputs see an infinity; the device saturates {len(extra)} more (first {extra[:3].tolist()}) and lacks {len(missing)}")
    assert int(want.sum()) == 2 * 4 * c.cout and torch.equal(hit, want), (len(extra), len(missing))
    assert torch.equal(got[0][~want], base[0][~want]), "an output outside the windows changed"
