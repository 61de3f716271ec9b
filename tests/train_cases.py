"""Case tables, operand builders and comparators for the training kernels' whole shape contract (tests/test_train_cases_host.py
on the host, tests/test_gpu_train_shapes.py on the MI355X).  A plain module: it imports without a device.

Integer probes.  Operands are small integers held in float64: x and dy in {-2..2}, w in {-1, 0, 1}, thinned by a density below 1
where a case needs it.  Every product and every partial sum, in any order, is then an exact integer, so an fp32 accumulator --
MFMA or not, split over workgroups or not -- returns exactly the float64 result as long as the sum of the absolute terms stays
below 2^24.  The builders assert sum |terms| <= 2^22 (EXACT_LIMIT) for every case and pass, taken as the maximum over the outputs
of the same operation on absolute values: two bits are kept spare because the alignment width inside the bf16 MFMA is not
documented.  It is a condition on the operands, not a measurement of any kernel.  The comparators are therefore zero-tolerance:
fp32 outputs equal the float64 reference, bf16 forward / dgrad outputs equal the float64 reference rounded once to bf16 (one
round-to-nearest-even of an exact sum is the rounding of the float64 value), bf16 wgrad (fp32 dW) equals it exactly.

Replicated batches.  A batch above 8 is built from D = 3 distinct samples and a seeded, non-periodic index list: x[b] = X[idx[b]],
dy[b] = DY[idx[b]].  The expected forward and dgrad outputs are REF[idx[b]], the expected wgrad is sum_d count_d * dW_d; the
float64 work stays at three samples and a kernel that reads the wrong sample or pairs x with the wrong dy is still caught."""

from collections import namedtuple

import torch
import torch.nn.functional as F

EXACT_LIMIT = 2 ** 22
D_SAMPLES = 3
FAMILIES = {"k1s1": (1, 1, 0), "k1s2": (1, 2, 0), "k3s1": (3, 1, 1), "k3s2": (3, 2, 1)}   # kernel, stride, padding
STEM = (7, 2, 3)
BATCHES = (1, 2, 3, 5)

# b: batch; cin / cout: the convolution's channels (a stem's cin is 6, 12 or 18: the functions pad it to 8, 16, 24); k, s, pad;
# h, w: input size; density: share of non-zero operand entries; seed
ConvCase = namedtuple("ConvCase", "b cin cout k s pad h w density seed")
BnCase = namedtuple("BnCase", "b h w c flags")   # rows = b * h * w


def conv_id(c: ConvCase) -> str:
    return f"b{c.b}-{c.cin}-{c.cout}-k{c.k}s{c.s}-{c.h}x{c.w}"


def bn_id(c: BnCase) -> str:
    return f"rows{c.b * c.h * c.w}({c.b}x{c.h}x{c.w})-c{c.c}-f{c.flags}"


def out_size(c: ConvCase):
    return (c.h + 2 * c.pad - c.k) // c.s + 1, (c.w + 2 * c.pad - c.k) // c.s + 1


def desc_tuple(c: ConvCase):
    """The fields of salve_conv_desc_t (salve_amd._lib.ConvDesc) for the case, input channels padded to a multiple of 8."""
    ho, wo = out_size(c)
    return (c.b, c.h, c.w, (c.cin + 7) // 8 * 8, ho, wo, c.cout, c.k, c.k, c.s, c.pad)


# ------------------------------------------------------------------------------------------------------------ convolution tables
SIZES = [(1, 1), (1, 9), (9, 1), (2, 3), (3, 2), (7, 12), (15, 8), (13, 29), (56, 40), (17, 130)]
M_EDGE = [(1, 127, 1), (2, 8, 8), (3, 43, 1)]   # (batch, H, W): batch * H * W = 127, 128, 129 around the 128-pixel tile edge
# (batch, Ho, Wo): batch * Ho * Wo around the 32-pixel wgrad tile edges 32, 256, 288, 544
P_EDGE = [(1, 1, 31), (2, 4, 4), (3, 11, 1), (5, 3, 17), (2, 8, 16), (1, 257, 1), (1, 7, 41), (3, 8, 12), (1, 17, 17), (3, 1, 181),
          (2, 16, 17), (5, 109, 1)]
P_VALUES = [31, 32, 33, 255, 256, 257, 287, 288, 289, 543, 544, 545]
CHANNELS = [(64, 64), (64, 128), (128, 64), (192, 64), (64, 192), (192, 320), (2048, 64), (64, 2048)]
STEM_CIN = [6, 12, 18]
STEM_SIZES = [(7, 7), (33, 65), (96, 160), (224, 224), (234, 300)]


def _conv_table():
    cases = []
    for fi, (k, s, pad) in enumerate(FAMILIES.values()):
        n = fi   # the batches {1, 2, 3, 5} rotate, from another start in every family

        def add(b, cin, cout, h, w):
            cases.append(ConvCase(b, cin, cout, k, s, pad, h, w, 1.0, len(cases)))

        for h, w in SIZES:
            add(BATCHES[n % 4], 64, 64, h, w)
            n += 1
        for b, h, w in M_EDGE:
            add(b, 64, 64, h, w)
        for i, (b, ho, wo) in enumerate(P_EDGE):   # stride 2: Ho = (H - 1) // 2 + 1 for both kernels; odd and even inputs alternate
            h, w = (ho, wo) if s == 1 else (2 * ho - (i & 1), 2 * wo - ((i >> 1) & 1))
            add(b, 64, 64, h, w)
        for i, (cin, cout) in enumerate(CHANNELS):
            h, w = ((7, 12), (9, 5))[i & 1]
            add(BATCHES[n % 4], cin, cout, h, w)
            n += 1
    n = 0
    for h, w in STEM_SIZES:
        for cin in STEM_CIN:
            cases.append(ConvCase(BATCHES[n % 4], cin, 64, *STEM, h, w, 1.0, len(cases)))
            n += 1
    return cases


CONV_CASES = _conv_table()

# Random normal operands against float64 with the existing tests' bounds: every family, every odd or non-square kind of shape.
RANDOM_CASES = [c for c in CONV_CASES if (c.k != 7 and (c.cin, c.cout) == (64, 64) and (c.h, c.w) in ((1, 9), (9, 1), (3, 2), (15, 8), (13, 29)))
                or (c.k != 7 and (c.cin, c.cout) == (192, 320)) or (c.k == 7 and (c.cin, c.h, c.w) in ((6, 33, 65), (12, 96, 160), (18, 7, 7)))]

# Batch 256 (replicated), one shape per kernel path.  The densities keep sum |terms| of the wgrad reduction (up to 3.2 M pixels)
# under EXACT_LIMIT; they were lowered, not the limit.
REAL_BATCH_CASES = [ConvCase(256, 64, 64, 3, 1, 1, 56, 56, 1.0, 1001), ConvCase(256, 128, 128, 3, 2, 1, 56, 56, 1.0, 1002),
                    ConvCase(256, 64, 256, 1, 1, 0, 56, 56, 1.0, 1003), ConvCase(256, 256, 512, 1, 2, 0, 56, 56, 1.0, 1004),
                    ConvCase(256, 512, 512, 3, 1, 1, 7, 7, 1.0, 1005), ConvCase(256, 12, 64, *STEM, 224, 224, 0.7, 1006)]

# Replicated 64 -> 64 @ 112 x 112 with tensors beyond 2^31 elements / 2^32 bytes.  fp32: batch 2700 = 33.9 M input pixels, 2.17 G
# input elements, 8.7 GB; the 1x1 / s1 output and both dgrads are as large.  bf16: batch 2800 = 2.25 G elements, 4.5 GB > 2^32
# bytes for the input, the 1x1 / s1 output and both dgrads.
LARGE_CASES = {"fp32": [ConvCase(2700, 64, 64, 1, 1, 0, 112, 112, 0.25, 2001), ConvCase(2700, 64, 64, 3, 2, 1, 112, 112, 0.5, 2002)],
               "bf16": [ConvCase(2800, 64, 64, 1, 1, 0, 112, 112, 0.25, 2003), ConvCase(2800, 64, 64, 3, 2, 1, 112, 112, 0.5, 2004)]}
LARGE_MIN_FREE_BYTES = 64 * 10 ** 9

# One representative case per family (and a stem) for the comparators' own test: batch >= 2, not square, 3 or more 8-channel chunks.
REPRESENTATIVE = {name: ConvCase(3, 64, 64, k, s, pad, 15, 10, 1.0, 3000 + i) for i, (name, (k, s, pad)) in enumerate(FAMILIES.items())}
REPRESENTATIVE["stem"] = ConvCase(2, 12, 64, *STEM, 33, 65, 1.0, 3010)
REPLICATED_REPRESENTATIVE = ConvCase(12, 64, 64, 3, 2, 1, 9, 6, 1.0, 3020)

# ------------------------------------------------------------------------------------------------------------ BatchNorm table
BN_RELU, BN_ADD = 1, 2   # salve_amd._lib.BN_RELU / BN_ADD (tests/test_train_cases_host.py checks the two against the library's)
BN_C = [8, 24, 72, 520, 4096]
BN_ROWS = [(1, 1, 2), (3, 1, 1), (1, 7, 7), (1, 257, 1), (1, 1, 12289)]   # rows 2, 3, 49, 257, 12,289


def _bn_table():
    """Every C with every row count; the four flag combinations rotate so that every C and every row count meets each of them,
    and (C = 520, rows = 12,289) and (C = 8, rows = 3) take all four."""
    cases = []
    for i, c in enumerate(BN_C):
        for j, (b, h, w) in enumerate(BN_ROWS):
            cases.append(BnCase(b, h, w, c, (i + j) % 4))
    for c, (b, h, w) in ((520, BN_ROWS[4]), (8, BN_ROWS[1])):
        cases += [BnCase(b, h, w, c, f) for f in range(4) if BnCase(b, h, w, c, f) not in cases]
    return cases


BN_CASES = _bn_table()
BN_REAL_BATCH_CASES = [BnCase(256, 7, 7, 2048, BN_ADD | BN_RELU), BnCase(256, 56, 56, 64, BN_RELU)]
BN_DETERMINISM_CASES = [BnCase(1, 1, 12289, 520, BN_ADD | BN_RELU), BnCase(3, 1, 1, 8, BN_ADD | BN_RELU)]


# ------------------------------------------------------------------------------------------------------------ operand builders
def _integers(shape, lo, hi, density, g):
    t = torch.randint(lo, hi + 1, shape, generator=g).double()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density)
    return t


def sample_index(c: ConvCase):
    """idx[b] of a replicated batch (None for a plain one): seeded, every sample used, no period."""
    if c.b <= 8:
        return None
    g = torch.Generator().manual_seed(7919 * c.seed + 1)
    idx = torch.randint(0, D_SAMPLES, (c.b,), generator=g)
    idx[:D_SAMPLES] = torch.arange(D_SAMPLES)
    assert all(not torch.equal(idx[p:], idx[:-p]) for p in range(1, min(c.b, 64)))
    return idx


def probe_operands(c: ConvCase):
    """x [n, cin, h, w], w [cout, cin, k, k], dy [n, cout, ho, wo] as integers in float64; n = batch, or D_SAMPLES for a
    replicated batch."""
    g = torch.Generator().manual_seed(c.seed)
    n = c.b if c.b <= 8 else D_SAMPLES
    ho, wo = out_size(c)
    x = _integers((n, c.cin, c.h, c.w), -2, 2, c.density, g)
    w = _integers((c.cout, c.cin, c.k, c.k), -1, 1, 1.0, g)
    dy = _integers((n, c.cout, ho, wo), -2, 2, c.density, g)
    return x, w, dy


def conv_passes(c: ConvCase, x, w, dy):
    """Float64 forward, dgrad (None for a stem) and per-sample wgrad [n, cout, cin, k, k] of the case's convolution."""
    fwd = F.conv2d(x, w, stride=c.s, padding=c.pad)
    dgrad = None if c.k == 7 else torch.nn.grad.conv2d_input(x.shape, w, dy, stride=c.s, padding=c.pad)
    if x.shape[0] > D_SAMPLES:   # a plain batch: only the sum is needed
        wgrad = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=c.s, padding=c.pad)[None]
    else:
        wgrad = torch.stack([torch.nn.grad.conv2d_weight(x[i:i + 1], w.shape, dy[i:i + 1], stride=c.s, padding=c.pad) for i in range(x.shape[0])])
    return fwd, dgrad, wgrad


def sum_wgrad(c: ConvCase, wgrad):
    """dW of the whole batch from conv_passes' wgrad: the plain sum, or sum_d count_d * dW_d for a replicated batch."""
    idx = sample_index(c)
    if idx is None:
        return wgrad.sum(0)
    counts = torch.bincount(idx, minlength=D_SAMPLES).double()
    return (wgrad * counts[:, None, None, None, None]).sum(0)


def abs_term_sums(c: ConvCase, x, w, dy):
    """max over outputs of sum |terms| for forward, dgrad and wgrad: the same operations on absolute values."""
    fwd, dgrad, wgrad = conv_passes(c, x.abs(), w.abs(), dy.abs())
    return {"fwd": float(fwd.max()), "dgrad": 0.0 if dgrad is None else float(dgrad.max()), "wgrad": float(sum_wgrad(c, wgrad).max())}


def build_probe(c: ConvCase):
    """Operands and float64 references of a probe case; asserts the exactness condition for each pass."""
    x, w, dy = probe_operands(c)
    for name, v in abs_term_sums(c, x, w, dy).items():
        assert v <= EXACT_LIMIT, (conv_id(c), name, v)
    fwd, dgrad, wgrad = conv_passes(c, x, w, dy)
    return {"x": x, "w": w, "dy": dy, "idx": sample_index(c), "fwd": fwd, "dgrad": dgrad, "wgrad": sum_wgrad(c, wgrad)}


def random_operands(c: ConvCase, bf16: bool):
    """test_conv_parity_against_float64's operands (test_bf16_conv_parity_against_float64's: rounded to bf16) at the case's shape."""
    g = torch.Generator().manual_seed(c.cin * 7 + c.cout + c.k * 13 + c.s + c.h + 1000 * c.w + c.b)
    rnd = (lambda t: t.to(torch.bfloat16).double()) if bf16 else (lambda t: t)
    x = rnd(torch.randn(c.b, c.cin, c.h, c.w, generator=g, dtype=torch.float64))
    w = rnd(torch.randn(c.cout, c.cin, c.k, c.k, generator=g, dtype=torch.float64) / (c.cin * c.k * c.k) ** 0.5)
    dy = rnd(torch.randn(c.b, c.cout, *out_size(c), generator=g, dtype=torch.float64))
    return x, w, dy


def make_bn_case(c: BnCase, dtype):
    """tests/test_gpu_train_norm.py::make_case's operands at a [b, c, h, w] that need not be square: x ~ N(mu_c, s_c) with mu_c up to
    30 and s_c in [0.5, 2], random gamma, beta, residual, dy and running statistics; dtype bfloat16 rounds the activations first."""
    g = torch.Generator().manual_seed(c.c * 31 + c.h * 7 + c.w * 13 + c.flags + c.b)
    shape = (c.b, c.c, c.h, c.w)
    mu = 30.0 * torch.rand(c.c, generator=g, dtype=torch.float64)
    s = 0.5 + 1.5 * torch.rand(c.c, generator=g, dtype=torch.float64)
    x = torch.randn(shape, generator=g, dtype=torch.float64) * s[None, :, None, None] + mu[None, :, None, None]
    res = torch.randn(shape, generator=g, dtype=torch.float64) if c.flags & BN_ADD else None
    dy = torch.randn(shape, generator=g, dtype=torch.float64)
    p = {"gamma": 0.5 + torch.rand(c.c, generator=g, dtype=torch.float64), "beta": torch.randn(c.c, generator=g, dtype=torch.float64),
         "rm": torch.randn(c.c, generator=g, dtype=torch.float64), "rv": 0.5 + torch.rand(c.c, generator=g, dtype=torch.float64)}
    p = {k: v.float().double() for k, v in p.items()}
    rnd = (lambda t: None if t is None else t.to(dtype).double())
    return rnd(x), rnd(res), rnd(dy), p


# ------------------------------------------------------------------------------------------------------------ comparators
def exact_f32(got, ref64) -> bool:
    """An fp32 output of an integer probe: exactly the float64 reference."""
    return got.dtype == torch.float32 and got.shape == ref64.shape and torch.equal(got.double(), ref64.to(got.device))


def exact_bf16(got, ref64) -> bool:
    """A bf16 output of an integer probe: the float64 reference rounded once to bf16."""
    return got.dtype == torch.bfloat16 and got.shape == ref64.shape and torch.equal(got, ref64.to(got.device).to(torch.bfloat16))


def exact_replicated(got, refs64, idx, compare=exact_f32, chunk: int = 64) -> bool:
    """got[b] against refs64[idx[b]] for every sample of a replicated batch, `chunk` samples at a time on got's device (upload the
    D references once; nothing the size of the batch is copied to the host)."""
    refs, idx = refs64.to(got.device), idx.to(got.device)
    if got.shape[0] != idx.shape[0]:
        return False
    return all(compare(got[i:i + chunk], refs[idx[i:i + chunk]]) for i in range(0, got.shape[0], chunk))


def replicate(samples, idx):
    """[D, C, H, W] -> the batch [B, C, H, W] with x[b] = samples[idx[b]], in channels_last memory (NHWC bytes), on samples' device."""
    return samples.permute(0, 2, 3, 1).contiguous()[idx.to(samples.device)].permute(0, 3, 1, 2)
