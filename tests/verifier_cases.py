"""Probes, a reference emulator, mutants and case tables for the fp16 verifier's kernels (tests/test_verifier_cases_host.py on the
host, tests/test_gpu_verifier_ops.py on the MI355X).  A plain module: it imports without a device.

Probes.  Operands are held in float64 and are representable in fp16: activations and residual sources are integers in {-2..2},
weights are in {-1, 0, 1} (thinned by a count of non-zero entries per row where a chain of ops has to stay alive without growing),
biases are multiples of QUANTUM = 2^-6.  Every product and every partial sum is then a multiple of 2^-6, and so is every stored
activation (an fp16 below 32 holds every multiple of 2^-6, above 32 its spacing is a multiple of it).  An fp32 accumulator -- MFMA or
not, in any order -- returns the exact sum as long as sum |terms| / 2^-6 <= 2^22: train_cases.EXACT_LIMIT, with the same two spare
bits for the undocumented alignment width inside the MFMA.  `check_exact` asserts that for every op of a program: the same op on
the absolute values of the buffers it really reads, of its weights, bias and residual.  The biases' fraction bits make the one rounding
at the fp16 store do work: values in [32, 64) with an odd count of 64ths are ties.

Emulator.  `Emulator` reads the arrays a `hip_resnet._Builder` packs -- the op records, the fp16 weight bits, the fp32 parameters and
the k table -- and runs the program buffer by buffer in float64.  A convolution's weight row is read THROUGH the k table (tap and
channel offset of every 8-element chunk), as conv_igemm_kernel reads it.  After each stored tensor: + bias, + residual, ReLU, saturate
to +-65504, ONE round-to-nearest-even to fp16 (resnet.hip: pack4_lo / f32_to_act).  With exact sums the result does not depend on the
summation order, so the comparators are zero-tolerance on the fp16 bits.

Mutants.  The emulator with one deliberate mistake each (MUTANTS); the host test asserts that every probe of the families a mutant
applies to tells it from the true emulator."""

from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import train_cases
from salve_amd.models import hip_resnet
from salve_amd.models.hip_resnet import NET_INPUT, NO_BUF, OP_AVGPOOL_FC, OP_CONV, OP_MAXPOOL

EXACT_LIMIT = train_cases.EXACT_LIMIT
QUANTUM = 2.0 ** -6
FP16_MAX = 65504.0
NAN_BITS = 0x7E00   # the fill of the workspace: an fp16 NaN

# flags of salve_resnet_create (salve_amd._lib.RESNET_*; the host test checks the values against the bindings')
IGEMM_ONLY, CONV8_WHEREVER, NO_STEM_FUSE, NO_BLOCK_FUSE, NO_CHAIN, NO_NEXT_FUSE = 1, 2, 8, 16, 64, 4096

MUTANTS = ("taps_transposed", "padding_is_a_pixel", "m_tile_edge_row", "stem_groups_swapped", "residual_after_relu", "round_half_away",
           "maxpool_zero_padding", "src2_stride_1", "avgpool_wrong_hw")


# ------------------------------------------------------------------------------------------------------------ rounding
def round_fp16(v: torch.Tensor, mode: str = "even") -> torch.Tensor:
    """float64 -> the nearest fp16 value, as float64: saturate to +-65504, then one rounding at 11 significand bits (spacing 2^-24
    below 2^-14), ties to even -- or away from zero (the mutant)."""
    v = v.clamp(-FP16_MAX, FP16_MAX)
    a = v.abs()
    _, ex = torch.frexp(a)                       # a = m * 2^ex, m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(a), ex.clamp(min=-13) - 11)
    q = a / ulp
    r = torch.round(q) if mode == "even" else torch.floor(q + 0.5)
    return torch.sign(v) * r * ulp


def fp16_bits(v: torch.Tensor) -> torch.Tensor:
    """An fp16-representable float64 tensor -> its int16 bit patterns."""
    h = v.to(torch.float16)
    assert torch.equal(h.double(), v), "not representable in fp16"
    return h.view(torch.int16)


# ------------------------------------------------------------------------------------------------------------ emulator
def pack(bld):
    """A _Builder's program as the arrays salve_resnet_create takes: (ops, weight bits, params, ktab)."""
    z = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(1, dt)
    return np.array(bld.ops, dtype=hip_resnet.OP_DTYPE), z(bld.weights, np.int16), z(bld.params, np.float32), z(bld.ktab, np.int32)


class Emulator:
    """rounding: "even" (the kernels'), "away" or None (no rounding and no saturation: the plain float64 operation).
    absolute: |weights|, |biases| -- run on |x| it gives sum |terms| of every op.  mutant: one of MUTANTS; m_tile: the M tile of the
    m_tile_edge_row mutant (128: conv_igemm_kernel, 256: conv8_kernel)."""

    def __init__(self, ops, weights, params, ktab, rounding="even", absolute=False, mutant=None, m_tile=128):
        assert mutant is None or mutant in MUTANTS
        self.ops, self.weights, self.params, self.ktab = ops, weights, params, ktab
        self.rounding = "away" if mutant == "round_half_away" else rounding
        self.absolute, self.mutant, self.m_tile = absolute, mutant, m_tile
        self.max_sum = 0.0      # largest |value| before the rounding (absolute: largest sum |terms|)
        self.max_stored = 0.0   # largest |stored value|

    def _a(self, t):
        return t.abs() if self.absolute else t

    def _store(self, v):
        self.max_sum = max(self.max_sum, float(v.abs().max()))
        out = v if self.rounding is None else round_fp16(v, self.rounding)
        self.max_stored = max(self.max_stored, float(out.abs().max()))
        return out

    def conv_weights(self, o):
        """[Cout, Cin, KH, KW] of the op's first source, placed by the k table, and [Cout, Cin2] of its second (or None)."""
        cout, cin, kh, kw = int(o["Cout"]), int(o["Cin"]), int(o["KH"]), int(o["KW"])
        k1 = kh * kw * cin
        cin2 = int(o["Cin2"]) if o["in2_buf"] != NO_BUF else 0
        k = k1 + cin2
        rows = self.weights[int(o["w_off"]): int(o["w_off"]) + cout * k].view(np.float16).astype(np.float64).reshape(cout, k)
        tab = self.ktab[int(o["ktab_off"]): int(o["ktab_off"]) + k1 // 8]
        w = np.zeros((cout, cin, kh, kw))
        if cin2:                                   # the point-wise kernels do not read the table: k is the channel
            w[:, :, 0, 0] = rows[:, :k1]
        else:
            for q, e in enumerate(tab):
                dy, dx, c0 = int(e) & 0xFF, (int(e) >> 8) & 0xFF, (int(e) >> 16) & 0xFFFF
                if self.mutant == "stem_groups_swapped" and kh == 7 and cin in (16, 24):
                    c0 = {0: 8, 8: 0}.get(c0, c0)
                w[:, c0:c0 + 8, dy, dx] += rows[:, 8 * q: 8 * q + 8]
        if self.mutant == "taps_transposed":
            n = min(kh, kw)
            w[:, :, :n, :n] = w[:, :, :n, :n].transpose(0, 1, 3, 2).copy()
        return self._a(torch.from_numpy(w)), (self._a(torch.from_numpy(rows[:, k1:].copy())) if cin2 else None)

    def conv(self, o, bufs):
        x = bufs[int(o["in_buf"])].permute(0, 3, 1, 2)
        hi, wi, ho, wo = int(o["Hi"]), int(o["Wi"]), int(o["Ho"]), int(o["Wo"])
        kh, kw, s, pad = int(o["KH"]), int(o["KW"]), int(o["stride"]), int(o["pad"])
        assert tuple(x.shape[1:]) == (int(o["Cin"]), hi, wi), (tuple(x.shape), o)
        w, w2 = self.conv_weights(o)
        need_h, need_w = (ho - 1) * s + kh, (wo - 1) * s + kw      # the extent the taps reach, from -pad on
        mode = "replicate" if self.mutant == "padding_is_a_pixel" and pad > 0 else "constant"
        xp = F.pad(x, (pad, max(need_w - wi - pad, 0), pad, max(need_h - hi - pad, 0)), mode=mode)[:, :, :need_h, :need_w]
        y = F.conv2d(xp, w, stride=s)
        if w2 is not None:
            x2, s2 = bufs[int(o["in2_buf"])].permute(0, 3, 1, 2), int(o["stride2"])
            assert tuple(x2.shape[1:]) == (int(o["Cin2"]), int(o["Hi2"]), int(o["Wi2"]))
            x2 = x2[:, :, :ho, :wo] if self.mutant == "src2_stride_1" else x2[:, :, ::s2, ::s2]
            y = y + F.conv2d(x2, w2[:, :, None, None])
        y = y.permute(0, 2, 3, 1).contiguous()
        assert tuple(y.shape[1:]) == (ho, wo, int(o["Cout"]))
        if self.mutant == "m_tile_edge_row" and y.shape[0] * ho * wo >= self.m_tile:
            flat = y.reshape(-1, y.shape[-1])
            rows = torch.arange(self.m_tile - 1, flat.shape[0], self.m_tile)
            flat[rows] = flat[rows - 1].clone()
        v = y + self._a(torch.from_numpy(self.params[int(o["b_off"]): int(o["b_off"]) + int(o["Cout"])].astype(np.float64)))
        res = bufs[int(o["res_buf"])] if o["res_buf"] != NO_BUF else None
        if res is not None and self.mutant != "residual_after_relu":
            v = v + res
        if o["relu"]:
            v = v.clamp(min=0)
        if res is not None and self.mutant == "residual_after_relu":
            v = v + res
        return self._store(v)

    def maxpool(self, o, bufs):
        x = bufs[int(o["in_buf"])].permute(0, 3, 1, 2)
        if self.mutant == "maxpool_zero_padding":
            y = F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 2, 0)
        else:
            y = F.max_pool2d(x, 3, 2, 1)
        assert tuple(y.shape[2:]) == (int(o["Ho"]), int(o["Wo"]))
        return self._store(y.permute(0, 2, 3, 1).contiguous())

    def fc(self, o, bufs):
        x = bufs[int(o["in_buf"])]
        c, ncls, hw = int(o["Cin"]), int(o["Cout"]), int(o["Hi"]) * int(o["Wi"])
        w = self._a(torch.from_numpy(self.params[int(o["w_off"]): int(o["w_off"]) + ncls * c].astype(np.float64).reshape(ncls, c)))
        b = self._a(torch.from_numpy(self.params[int(o["b_off"]): int(o["b_off"]) + ncls].astype(np.float64)))
        mean = x.reshape(x.shape[0], hw, c).sum(1) / (hw + 1 if self.mutant == "avgpool_wrong_hw" else hw)
        logits = mean @ w.T + b
        self.max_sum = max(self.max_sum, float((mean.abs() @ w.abs().T + b.abs()).max()))
        return logits

    def run_op(self, i, bufs):
        o = self.ops[i]
        return {OP_CONV: self.conv, OP_MAXPOOL: self.maxpool, OP_AVGPOOL_FC: self.fc}[int(o["op"])](o, bufs)

    def run(self, x, before_op=None):
        """x: NHWC float64 network input -> (final buffer contents {buffer: NHWC tensor}, logits or None, per-op outputs)."""
        bufs, logits, stores = {NET_INPUT: self._a(x)}, None, []
        for i, o in enumerate(self.ops):
            if before_op:
                before_op(i, bufs)
            out = self.run_op(i, bufs)
            stores.append(out)
            if int(o["op"]) == OP_AVGPOOL_FC:
                logits = out
            else:
                bufs[int(o["out_buf"])] = out
        return bufs, logits, stores


# ------------------------------------------------------------------------------------------------------------ programs
# bld: the _Builder; x: NHWC float64 input (padded channels zero); read: {buffer: (H, W, C)} of the buffers that can be compared at the
# end of the program under every kernel selection; even: the buffer whose odd pixels stay unwritten in the even-pixel forms (or None)
Program = namedtuple("Program", "name bld x read even")


def emulate(prog, **kw):
    return Emulator(*pack(prog.bld), **kw).run(prog.x)


def check_exact(prog):
    """The probe condition of every op of the program, and no stored value at the fp16 limit.  Returns the true emulation."""
    arrays = pack(prog.bld)
    true, terms = Emulator(*arrays), Emulator(*arrays, rounding=None, absolute=True)
    out = true.run(prog.x, before_op=lambda i, bufs: terms.run_op(i, {k: v.abs() for k, v in bufs.items()}))
    assert terms.max_sum / QUANTUM <= EXACT_LIMIT, (prog.name, terms.max_sum)   # sum |terms| of every op on the inputs it really gets
    assert true.max_stored < FP16_MAX, (prog.name, true.max_stored)
    for i, t in enumerate(out[2]):
        assert torch.equal(t, torch.round(t / QUANTUM) * QUANTUM), (prog.name, i, "a stored value is no multiple of 2^-6")
    return out


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _weights(g, cout, cin, k, nz=None):
    """{-1, 0, 1}; nz: the mean count of non-zero entries per output channel (None: two thirds of them)."""
    if nz is None:
        return _ints(g, (cout, cin, k, k), -1, 1)
    sign = 2 * _ints(g, (cout, cin, k, k), 0, 1) - 1
    return sign * (torch.rand(sign.shape, generator=g) < nz / (cin * k * k))


def _bias(g, cout, lo, hi):
    """Multiples of 2^-6 with magnitudes in [lo, hi), either sign."""
    n = torch.randint(int(lo / QUANTUM), int(hi / QUANTUM), (cout,), generator=g).double() * QUANTUM
    return n * (2 * torch.randint(0, 2, (cout,), generator=g).double() - 1)


def _input(g, b, h, w, cin):
    x = torch.zeros(b, h, w, hip_resnet.pad_channels(cin), dtype=torch.float64)
    x[..., :cin] = _ints(g, (b, h, w, cin), -2, 2)
    return x


def _random_input(g, b, h, w, cin):
    x = torch.zeros(b, h, w, hip_resnet.pad_channels(cin), dtype=torch.float64)
    x[..., :cin] = torch.randn(b, h, w, cin, generator=g).to(torch.float16).double()
    return x


# ---- single convolutions
# cin: the real input channels (a stem's 6, 12, 18 are padded to 8, 16, 24); kw_pad: 8 for a table with 8 slots per kernel row;
# res: a producer (1x1 / stride s, no ReLU) writes a residual; src2: None or (cin2, stride2) -- then the op is the last 1x1 of a
# down-sampling block: a 3x3 / stride2 producer cin2 -> cin writes its first source, the input itself is the second
VCase = namedtuple("VCase", "b cin cout k s pad h w relu res kw_pad src2 seed")


def case_id(c: VCase) -> str:
    tail = ("-relu" if c.relu else "") + ("-res" if c.res else "") + (f"-src2({c.src2[0]},s{c.src2[1]})" if c.src2 else "")
    return f"b{c.b}-{c.cin}-{c.cout}-k{c.k}s{c.s}-{c.h}x{c.w}{tail}"


def out_size(c: VCase):
    if c.src2:
        return (c.h - 1) // c.src2[1] + 1, (c.w - 1) // c.src2[1] + 1
    return (c.h + 2 * c.pad - c.k) // c.s + 1, (c.w + 2 * c.pad - c.k) // c.s + 1


def conv_program(c: VCase, random: bool = False) -> Program:
    """The case as a program: [producer,] convolution.  Buffer 0 is the convolution's output unless the case has a second source
    (then buffer 0 is the producer's, buffer 1 the output); a residual is buffer 1.  random: normal operands rounded to fp16
    (weights scaled by the fan-in) instead of the probes."""
    g = torch.Generator().manual_seed(c.seed * 2 + int(random))
    bld = hip_resnet._Builder()
    ho, wo = out_size(c)
    x = (_random_input if random else _input)(g, c.b, c.h, c.w, c.src2[0] if c.src2 else c.cin)

    def wt(cout, cin, k, nz=None):
        return torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5 if random else _weights(g, cout, cin, k, nz)

    def bs(cout, lo=32.0, hi=64.0):
        return torch.randn(cout, generator=g) * 0.1 if random else _bias(g, cout, lo, hi)

    if c.src2:
        cin2, s2 = c.src2
        bld.conv(wt(c.cin, cin2, 3, 8), bs(c.cin, 0.0, 1.0), NET_INPUT, 0, NO_BUF, c.h, c.w, s2, 1, True)
        bld.conv1x1_with_shortcut(wt(c.cout, c.cin, 1), bs(c.cout, 16.0, 32.0), 0, 1, ho, wo, wt(c.cout, cin2, 1), bs(c.cout, 16.0, 32.0), NET_INPUT, c.h, c.w, s2)
        return Program(case_id(c), bld, x, {0: (ho, wo, c.cin), 1: (ho, wo, c.cout)}, None)
    read = {0: (ho, wo, c.cout)}
    if c.res:
        bld.conv(wt(c.cout, c.cin, 1, 6), bs(c.cout, 0.0, 4.0), NET_INPUT, 1, NO_BUF, c.h, c.w, c.s, 0, False)
        read[1] = (ho, wo, c.cout)
    bld.conv(wt(c.cout, c.cin, c.k), bs(c.cout), NET_INPUT, 0, 1 if c.res else NO_BUF, c.h, c.w, c.s, c.pad, bool(c.relu), c.kw_pad)
    return Program(case_id(c), bld, x, read, None)


FAMILIES = {"k1s1": (1, 1, 0), "k3s1": (3, 1, 1), "k3s2": (3, 2, 1), "k1s2_linear": (1, 2, 0)}   # kernel, stride, padding
SIZES = train_cases.SIZES
M_EDGE = train_cases.M_EDGE                    # (batch, Ho, Wo): 127, 128, 129 output pixels
M_EDGE_256 = [(1, 255, 1), (1, 16, 16), (1, 257, 1)]   # 255, 256, 257
CHANNELS = [(64, 64), (64, 128), (128, 64), (192, 64), (64, 192), (192, 320)]
STEM_CIN = train_cases.STEM_CIN


def _conv_table():
    cases, n = {name: [] for name in FAMILIES}, 0
    for fi, (name, (k, s, pad)) in enumerate(FAMILIES.items()):
        n = fi   # batches, ReLU and residual rotate, from another start in every family

        def add(b, cin, cout, h, w, kw_pad=0):
            i = len(cases[name])
            relu = 0 if name == "k1s2_linear" else (i + fi) % 3 != 2          # mostly on: a residual under a ReLU is the blocks' form
            res = cin % 64 == 0 and (i + fi) % 2 == 0
            cases[name].append(VCase(b, cin, cout, k, s, pad, h, w, int(relu), int(res), kw_pad, None, 100 * fi + i))

        for h, w in SIZES:
            add(train_cases.BATCHES[n % 4], 64, 64, h, w)
            n += 1
        for b, ho, wo in M_EDGE:   # stride 2: Ho = (H - 1) // 2 + 1 for both kernels
            add(b, 64, 64, *((ho, wo) if s == 1 else (2 * ho - 1, 2 * wo - (wo > 1))))
        for i, (cin, cout) in enumerate(CHANNELS):
            add(train_cases.BATCHES[n % 4], cin, cout, *((7, 12), (9, 5))[i & 1])
            n += 1
        if k == 3:
            add(2, 24, 64, 7, 12, kw_pad=8)    # three chunks per tap, eight table slots per kernel row
            add(3, 512, 512, 5, 3)
    return cases


CONV_CASES = _conv_table()
STEM_CASES = [VCase(train_cases.BATCHES[i % 4], STEM_CIN[i % 3], 64, 7, 2, 3, h, w, 1, 0, 8, None, 500 + i) for i, (h, w) in enumerate(SIZES)] + \
             [VCase(2, cin, 64, 7, 2, 3, 33, 65, 1, 0, 8, None, 520 + i) for i, cin in enumerate(STEM_CIN)]
# the last 1x1 of a down-sampling block with the projection shortcut as its second source: Cout 64 and 192 take BN = 64, 256 takes 128
SRC2_CASES = [VCase(b, 64, cout, 1, 1, 0, h, w, 1, 0, 0, (cin2, s2), 600 + i) for i, (b, cout, cin2, s2, h, w) in enumerate([
    (2, 64, 64, 1, 7, 12), (3, 64, 128, 2, 13, 29), (1, 192, 64, 2, 9, 1), (5, 192, 64, 1, 3, 2), (2, 256, 64, 1, 15, 8), (3, 256, 128, 2, 13, 29),
    (1, 64, 64, 1, 127, 1), (2, 192, 64, 2, 15, 16), (3, 256, 64, 1, 43, 1), (1, 192, 192, 2, 1, 9)])]
# shapes conv8_kernel accepts (Cout % 256 == 0, Cin a power of two >= 64, K >= 128) around its 256-pixel tile: point-wise, gather, second source
CONV8_CASES = [VCase(b, cin, cout, k, 1, k // 2, h, w, relu, res, 0, None, 700 + i) for i, (b, h, w) in enumerate(M_EDGE_256)
               for cin, cout, k, relu, res in ((128, 256, 1, 1, 1), (64, 512, 3, 0, 0), (256, 512, 1, 0, 1), (64, 256, 3, 1, 1))] + \
              [VCase(b, 64, cout, 1, 1, 0, h, w, 1, 0, 0, (64, 1), 760 + i) for i, ((b, h, w), cout) in enumerate(zip(M_EDGE_256, (256, 512, 256)))]
ALL_CONV_CASES = [c for fam in CONV_CASES.values() for c in fam] + STEM_CASES + SRC2_CASES + CONV8_CASES

# Random normal operands against float64: one odd non-square case per family, (192, 320), the three stems, a second source.
RANDOM_CASES = [c for fam in CONV_CASES.values() for c in fam if (c.cin, c.cout, c.h, c.w) == (64, 64, 13, 29) or (c.cin, c.cout) == (192, 320)] + \
               STEM_CASES[-3:] + [SRC2_CASES[1], SRC2_CASES[2]]

# A 3x3 / stride 2 gather without ReLU for the non-finite test: (case, the two interior pixels [b, y, x] that hold an infinity; odd
# coordinates: four windows each)
NON_FINITE_CASE = (VCase(2, 64, 64, 3, 2, 1, 13, 29, 0, 0, 0, None, 900), [(0, 5, 13), (1, 3, 21)])


def mutant_applies(m: str, c: VCase) -> bool:
    """Whether the conv case can see the mutant at all (a 1 x 1 image meets only the centre tap: nothing to transpose)."""
    ho, wo = out_size(c)
    return {"taps_transposed": c.k > 1 and not c.src2 and (c.h > 1 or c.w > 1),"padding_is_a_pixel": c.pad > 0 and not c.src2,
            "m_tile_edge_row": c.b * ho * wo >= 128, "stem_groups_swapped": c.k == 7 and c.cin > 8, "residual_after_relu": bool(c.res and c.relu),
            "round_half_away": True, "src2_stride_1": bool(c.src2) and c.src2[1] == 2 and (c.h > 1 or c.w > 1)}.get(m, False)


# ---- max-pool and average pool + classifier
PoolCase = namedtuple("PoolCase", "b h w c seed")
FcCase = namedtuple("FcCase", "b h w c ncls seed")
MAXPOOL_CASES = [PoolCase(train_cases.BATCHES[(i + j) % 4], h, w, c, 1000 + 10 * i + j) for i, c in enumerate((8, 64, 72))
                 for j, (h, w) in enumerate([(1, 1), (1, 9), (9, 1), (2, 3), (3, 2), (4, 4), (8, 6), (7, 12), (15, 8), (13, 29)])]
FC_SIZES = [(1, 1), (2, 2), (1, 4), (4, 4), (2, 8), (8, 8), (7, 7), (5, 7)]   # HW 1, 4, 4, 16, 16, 64 (1 / HW exact); 49, 35
FC_CASES = [FcCase(train_cases.BATCHES[(i + j) % 4], h, w, c, (1, 2, 3, 8)[(i + j) % 4], 1100 + 10 * i + j) for i, (h, w) in enumerate(FC_SIZES)
            for j, c in enumerate((8, 512, 2048, 2056, 4096))]


def pool_id(c):
    return f"b{c.b}-{c.h}x{c.w}-c{c.c}" + (f"-n{c.ncls}" if hasattr(c, "ncls") else "")


def maxpool_program(c: PoolCase) -> Program:
    """Multiples of 2^-6 of either sign; a band of two pixels along every border is all negative, so every window that touches the
    padding holds negative values only (the padding is minus infinity, not zero)."""
    g = torch.Generator().manual_seed(c.seed)
    x = _ints(g, (c.b, c.h, c.w, c.c), -512, 512) * QUANTUM
    band = torch.zeros(c.h, c.w, dtype=torch.bool)
    band[:2], band[-2:], band[:, :2], band[:, -2:] = True, True, True, True
    x = torch.where(band[None, :, :, None], -x.abs() - QUANTUM, x)
    bld = hip_resnet._Builder()
    ho, wo = bld.maxpool(NET_INPUT, 0, c.h, c.w, c.c)
    return Program(pool_id(c), bld, x, {0: (ho, wo, c.c)}, None)


def fc_exact(c: FcCase) -> bool:
    hw = c.h * c.w
    return hw & (hw - 1) == 0


def fc_program(c: FcCase) -> Program:
    """1 / HW exact: integer activations, classifier weights in {-1, 0, 1}, biases in 64ths -- the logits are exact in fp32.  Otherwise
    normal activations (fp16) and fp32 normal classifier parameters, for the comparison with a tolerance."""
    g = torch.Generator().manual_seed(c.seed)
    bld = hip_resnet._Builder()
    if fc_exact(c):
        x = _ints(g, (c.b, c.h, c.w, c.c), -2, 2)
        bld.fc(_ints(g, (c.ncls, c.c), -1, 1), _bias(g, c.ncls, 0.0, 8.0), NET_INPUT, c.h, c.w, c.c)
    else:
        x = torch.randn(c.b, c.h, c.w, c.c, generator=g).to(torch.float16).double()
        bld.fc(torch.randn(c.ncls, c.c, generator=g) / c.c ** 0.5, torch.randn(c.ncls, generator=g) * 0.1, NET_INPUT, c.h, c.w, c.c)
    return Program(pool_id(c), bld, x, {}, None)


# ---- the fused 56 x 56 block
BLOCK_SIZES = [(8, 8), (8, 16), (16, 20), (8, 13), (24, 40), (16, 56), (56, 56)]
BLOCK_BATCHES = (1, 3)
NEW_WIDTH_BLOCKS = [(8, 8), (16, 20), (8, 13)]   # tiles_x = 0; a partly empty last tile column at W % 8 != 0 and at an odd W


def block_program(h: int, w: int, b: int) -> Program:
    """test_fused_block_outputs_are_bit_identical_tensor_for_tensor's program on probes: producer, projection block, plain block, the
    next block's first 1x1, and the stride-2 block that reads Y (buffer 4) through its shortcut.  About eight non-zero weights per
    row keep the ten stores alive and small."""
    g = torch.Generator().manual_seed(h * 100 + w + b)
    bld = hip_resnet._Builder()
    wt = lambda cout, cin, k: _weights(g, cout, cin, k, 8)
    bs = lambda cout: _bias(g, cout, 0.0, 2.0)
    bld.conv(wt(64, 64, 1), bs(64), NET_INPUT, 0, NO_BUF, h, w, 1, 0, True)
    bld.conv(wt(64, 64, 1), bs(64), 0, 1, NO_BUF, h, w, 1, 0, True)
    bld.conv(wt(64, 64, 3), bs(64), 1, 2, NO_BUF, h, w, 1, 1, True)
    bld.conv1x1_with_shortcut(wt(256, 64, 1), bs(256), 2, 3, h, w, wt(256, 64, 1), bs(256), 0, h, w, 1)
    bld.conv(wt(64, 256, 1), bs(64), 3, 1, NO_BUF, h, w, 1, 0, True)
    bld.conv(wt(64, 64, 3), bs(64), 1, 2, NO_BUF, h, w, 1, 1, True)
    bld.conv(wt(256, 64, 1), bs(256), 2, 4, 3, h, w, 1, 0, True)
    bld.conv(wt(128, 256, 1), bs(128), 4, 1, NO_BUF, h, w, 1, 0, True)
    ho, wo = bld.conv(wt(128, 128, 3), bs(128), 1, 2, NO_BUF, h, w, 2, 1, True)
    bld.conv1x1_with_shortcut(wt(512, 128, 1), bs(512), 2, 0, ho, wo, wt(512, 256, 1), bs(512), 4, h, w, 2)
    read = {3: (h, w, 256), 4: (h, w, 256), 1: (h, w, 128), 2: (ho, wo, 128), 0: (ho, wo, 512)}
    return Program(f"block-b{b}-{h}x{w}", bld, _input(g, b, h, w, 64), read, 4 if h == w else None)


# ---- expand + chain
# (mid, midn): (128, 256) is the chained form that stores Y's even pixels at square even sizes; (128, 128) and (256, 256) the other chained
# forms; (256, 128) and (128, 64) have no chained form: expand only
CHAIN_CASES = [(128, 256, b, h, w) for b, h, w in [(2, 8, 8), (1, 16, 16), (1, 12, 12), (3, 43, 1), (1, 257, 1), (1, 127, 1), (5, 17, 3)]] + \
              [(128, 128, 2, 8, 8), (128, 128, 3, 5, 17), (256, 256, 1, 16, 16), (256, 256, 3, 43, 1), (256, 128, 1, 12, 12), (128, 64, 1, 127, 1),
               (128, 64, 2, 8, 8)]


def chain_program(mid: int, midn: int, b: int, h: int, w: int) -> Program:
    """X = 1x1 of the input; t1 = 1x1 of X; t2 = 3x3 mid -> mid; Y = relu(expand(t2) + X); the next block's reduce 4 mid -> midn of Y; its
    3x3 / stride 2; its last 1x1 with the stride-2 projection shortcut reading Y (buffer 3)."""
    g = torch.Generator().manual_seed(mid * 7 + midn + 1000 * h + w + b)
    bld = hip_resnet._Builder()
    wt = lambda cout, cin, k: _weights(g, cout, cin, k, 8)
    bs = lambda cout: _bias(g, cout, 0.0, 2.0)
    bld.conv(wt(4 * mid, 64, 1), bs(4 * mid), NET_INPUT, 0, NO_BUF, h, w, 1, 0, True)
    bld.conv(wt(mid, 4 * mid, 1), bs(mid), 0, 1, NO_BUF, h, w, 1, 0, True)
    bld.conv(wt(mid, mid, 3), bs(mid), 1, 2, NO_BUF, h, w, 1, 1, True)
    bld.conv(wt(4 * mid, mid, 1), bs(4 * mid), 2, 3, 0, h, w, 1, 0, True)
    bld.conv(wt(midn, 4 * mid, 1), bs(midn), 3, 1, NO_BUF, h, w, 1, 0, True)
    ho, wo = bld.conv(wt(midn, midn, 3), bs(midn), 1, 2, NO_BUF, h, w, 2, 1, True)
    bld.conv1x1_with_shortcut(wt(4 * midn, midn, 1), bs(4 * midn), 2, 4, ho, wo, wt(4 * midn, 4 * mid, 1), bs(4 * midn), 3, h, w, 2)
    read = {0: (h, w, 4 * mid), 3: (h, w, 4 * mid), 1: (h, w, midn), 2: (ho, wo, midn), 4: (ho, wo, 4 * midn)}
    even = 3 if (mid, midn) == (128, 256) and h == w and h % 2 == 0 else None
    return Program(f"chain-{mid}-{midn}-b{b}-{h}x{w}", bld, _input(g, b, h, w, 64), read, even)


# ---- stem + max-pool
STEM_POOL_CASES = [(cin, h, (1, 2, 3)[(i + j) % 3]) for i, cin in enumerate(STEM_CIN) for j, h in enumerate((16, 32, 48))]


def stem_program(cin: int, h: int, b: int) -> Program:
    """The 7x7 / 2 stem (k table with 8 slots per kernel row; 12 and 18 channels packed group-major) and the 3x3 / 2 max-pool at W = 224.
    Buffer 0 (the un-pooled convolution) exists only on the two-kernel path."""
    g = torch.Generator().manual_seed(cin * 100 + h + b)
    bld = hip_resnet._Builder()
    ho, wo = bld.conv(_weights(g, 64, cin, 7), _bias(g, 64, 32.0, 64.0), NET_INPUT, 0, NO_BUF, h, 224, 2, 3, True, 8)
    hp, wp = bld.maxpool(0, 1, ho, wo, 64)
    return Program(f"stem-{cin}-b{b}-{h}x224", bld, _input(g, b, h, 224, cin), {0: (ho, wo, 64), 1: (hp, wp, 64)}, None)


# ------------------------------------------------------------------------------------------------------------ comparators
def diff_report(got_bits: torch.Tensor, want_bits: torch.Tensor, what: str, limit: int = 5) -> str:
    """'' if the int16 tensors agree, else the count and the first few differing [b, y, x, c] with both values."""
    if got_bits.shape != want_bits.shape:
        return f"{what}: shape {tuple(got_bits.shape)} against {tuple(want_bits.shape)}"
    bad = (got_bits != want_bits).nonzero()
    if len(bad) == 0:
        return ""
    first = [(idx.tolist(), float(got_bits[tuple(idx)].view(torch.float16)), float(want_bits[tuple(idx)].view(torch.float16))) for idx in bad[:limit]]
    return f"{what}: {len(bad)} of {got_bits.numel()} values differ; first [b, y, x, c] (got, want): {first}"


def rounded_bound(r: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """The fp16 form of the project's check_rounded: half an fp16 ulp of the reference, the fp32 accumulation term on the same operation
    over absolute operands, the fp16 subnormal spacing."""
    return 2.0 ** -11 * r.abs() + 2.0 ** -20 * a + 2.0 ** -25
