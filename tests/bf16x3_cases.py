"""Shared by tests/test_bf16x3_host.py (CPU) and tests/test_gpu_verifier_bf16x3.py (GPU): the host emulation of the bf16x3 convolution
(salve_amd/csrc/conv_bf16x3.h) -- split every fp32 operand into two bf16 pieces, three fp32 conv2d over the pieces, fp32 activations --,
the float64 reference with its magnitude, the derived per-convolution bound, the convolution cases and the whole-network emulation.

The bound is derived, not measured: with |x - hi| <= 2^-9 |x| and |lo - bf16(lo)| <= 2^-9 |lo| each of the three pieces of one product
that the scheme drops or rounds (al * wl, and the residues of a and of w after two pieces) is <= 2^-18 |a| |w|; the fp32 accumulation gets
the 4e-6 x mag that tests/test_gpu_verifier_f32.py allows the fp32 engine.  mag = sum |a| |w| + |bias| (+ |residual|), in float64.
(2^-9 is the rounding error of a typical operand: bf16 keeps 8 significand bits, so an operand just above a power of two can lose 2^-8 and
a single product 2^-16 per piece.  A convolution output sums K such pieces of mixed sign and the emulation stays below 0.4 of the bound on
every case here, while losing a cross term exceeds it on every case -- test_bf16x3_host.py checks both.)"""

import torch

F = torch.nn.functional

BOUND_FACTOR = 3 * 2.0 ** -18 + 4e-6
BF16_MAX = float.fromhex("0x1.fep127")   # the largest finite bf16

# Default-BatchNorm ResNet-152 (activations ~1e8; tests: `default_bn_case`): max |logit error| / max |logit| of the host emulation
# against the fp32 oracle.  The GPU test allows 10 x this.
EMULATED_DEFAULT_BN_REL_ERR = 4.0e-6   # measured on the GPU engine (MI355X): 4.89e-6


def split(x):
    """fp32 tensor -> (hi, lo), both fp32 tensors holding bf16 values, by the engine's rules: hi = bf16(x) to nearest even, lo =
    bf16(x - hi); NaN -> (NaN, 0); +-inf -> (+-inf, 0) without computing inf - inf; a finite x that would round to inf -> hi = the
    largest finite bf16 of its sign."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    hi = torch.where(torch.isinf(hi) & torch.isfinite(x), torch.copysign(torch.full_like(x, BF16_MAX), x), hi)
    special = ~torch.isfinite(x)
    zero = torch.zeros_like(x)
    lo = (torch.where(special, zero, x) - torch.where(special, zero, hi)).to(torch.bfloat16).float()
    return hi, lo


TERMS_ALL = ("hh", "hl", "lh")
WRONG_KERNELS = {"no ah*wl": ("hh", "lh"), "no al*wh": ("hh", "hl"), "ah*wh only": ("hh",)}


def emu_conv(x, w, b, stride, pad, terms=TERMS_ALL):
    """The emulated convolution, NCHW in and out, fp32: the sum of the products named in `terms` (+ bias)."""
    ah, al = split(x)
    wh, wl = split(w)
    ops = {"hh": (ah, wh), "hl": (ah, wl), "lh": (al, wh)}
    out = None
    for t in terms:
        y = F.conv2d(ops[t][0], ops[t][1], None, stride, pad)
        out = y if out is None else out + y
    return out if b is None else out + b.float().view(1, -1, 1, 1)


def conv64(x, w, b, stride, pad):
    """float64 reference and sum |a| |w| + |bias| per output, NCHW in, NHWC out (as tests/test_gpu_verifier_f32.py::conv64)."""
    x, w = x.double(), w.double()
    ref = F.conv2d(x, w, b.double(), stride, pad)
    mag = F.conv2d(x.abs(), w.abs(), b.double().abs(), stride, pad)
    return ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def worst_ratio(got_nhwc, ref, mag, factor=BOUND_FACTOR):
    """max over the outputs of |got - ref| / (factor x mag): within the bound iff <= 1."""
    err = (got_nhwc.double() - ref).abs()
    return float((err / (factor * mag).clamp(min=1e-300)).max())


def rand_w(g, cout, cin, k):
    return torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5


# Single convolutions (tests/test_gpu_verifier_bf16x3.py runs each as a one-op program): stems on 34 x 34 at batch 2, then the plain ones.
CONV_CASES = [
    dict(name="stem6", cin=6, cout=64, k=7, s=2, p=3, hw=34, batch=2, relu=True, stem=True),
    dict(name="stem12", cin=12, cout=64, k=7, s=2, p=3, hw=34, batch=2, relu=True, stem=True),
    dict(name="stem18", cin=18, cout=64, k=7, s=2, p=3, hw=34, batch=2, relu=True, stem=True),
    dict(name="1x1-64-256", cin=64, cout=256, k=1, s=1, p=0, hw=14, batch=3, relu=False),
    dict(name="3x3-64-128-relu", cin=64, cout=128, k=3, s=1, p=1, hw=14, batch=3, relu=True),
    dict(name="3x3s2-64-64-odd", cin=64, cout=64, k=3, s=2, p=1, hw=15, batch=3, relu=True),      # odd size, the 64-wide tile
    dict(name="1x1s2-64-128", cin=64, cout=128, k=1, s=2, p=0, hw=15, batch=3, relu=False),
    dict(name="3x3-512-64-49px", cin=512, cout=64, k=3, s=1, p=1, hw=7, batch=1, relu=False),     # 49 pixels: less than one block tile
    dict(name="1x1-2048-64", cin=2048, cout=64, k=1, s=1, p=0, hw=7, batch=2, relu=False),
]


def case_tensors(case):
    """(x NCHW, w, b) of a convolution case, seeded by its name."""
    g = torch.Generator().manual_seed(sum(map(ord, case["name"])))
    w, b = rand_w(g, case["cout"], case["cin"], case["k"]), torch.randn(case["cout"], generator=g) * 0.1
    x = torch.randn(case["batch"], case["cin"], case["hw"], case["hw"], generator=g)
    return x, w, b


def case_reference(case, x, w, b):
    """(ref, mag) NHWC float64 of the case's output (ReLU applied to the reference where the case has one)."""
    ref, mag = conv64(x, w, b, case["s"], case["p"])
    return (ref.clamp(min=0) if case["relu"] else ref), mag


# `beyond_bf16_case`: its outputs at the huge inputs are ONE product each, so nothing averages and the worst case of a single product
# holds: a clamped operand keeps a whole ulp as residue (|a - ah| <= 2^-8 |a|), of which lo leaves 2^-9: 2^-17 |a|; the weight's residue
# is 2^-16 |w| at worst; the dropped al * wl is 2^-8 x 2^-8.  Sum: (2^-17 + 2 x 2^-16) |a| |w|, plus the fp32 accumulation's 4e-6.
BEYOND_BF16_BOUND_FACTOR = 2.0 ** -17 + 2 * 2.0 ** -16 + 4e-6


def beyond_bf16_case():
    """A 1 x 1 convolution, 64 -> 64 channels on 8 x 8, whose input holds finite values beyond the largest bf16 (+-FLT_MAX and 3.399e38:
    their hi piece is the clamped one) next to ordinary ones; weights of 2^-40 scale keep the fp32 outputs finite.  (case, x, w, b);
    the bound is BEYOND_BF16_BOUND_FACTOR x mag."""
    case = dict(name="beyond-bf16", cin=64, cout=64, k=1, s=1, p=0, hw=8, batch=1, relu=False)
    x, w, b = case_tensors(case)
    x[0, 5, 2, 3], x[0, 7, 4, 4], x[0, 9, 6, 1] = 3.399e38, -float.fromhex("0x1.fffffep127"), float.fromhex("0x1.fffffep127")
    return case, x, w * 2.0 ** -40, b * 2.0 ** -40


def tile_like_inputs(n, batch, seed=0):
    """n fp32 [batch, 3, 224, 224] tensors with the value set of real tiles: (v - mean) / std of uint8 values."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 256, (n, batch, 3, 224, 224), generator=g).float()
    mean = torch.tensor([123.675, 116.28, 103.53]).view(1, 1, 3, 1, 1)
    std = torch.tensor([58.395, 57.12, 57.375]).view(1, 1, 3, 1, 1)
    return list(((v - mean) / std).unbind(0))


def emu_forward(sd, num_layers, xs, terms=TERMS_ALL):
    """The whole network as the bf16x3 engine runs it: BatchNorm folded into fp32 weights and biases (hip_resnet.fold_bn), every
    convolution emulated by `emu_conv`, activations, residual adds, pools and the head in fp32."""
    from salve_amd.models.hip_resnet import _bn, fold_bn
    from salve_amd.models.resnet_factory import RESNET_SPECS

    sd = {(k[7:] if k.startswith("module.") else k): v.detach().float().cpu() for k, v in sd.items()}
    kind, blocks = RESNET_SPECS[num_layers]

    def conv(x, wkey, bnkey, stride=1, pad=0):
        w, b = fold_bn(sd[wkey], _bn(sd, bnkey))
        return emu_conv(x, w, b, stride, pad, terms)

    x = torch.cat(xs, dim=1).float()
    x = F.max_pool2d(F.relu(conv(x, "conv1.weight", "resnet.bn1", 2, 3)), 3, 2, 1)
    for si, n in enumerate(blocks):
        for bi in range(n):
            p = f"resnet.layer{si + 1}.{bi}"
            stride = 2 if (bi == 0 and si > 0) else 1
            idn = x
            if kind == "bottleneck":
                o = F.relu(conv(x, f"{p}.conv1.weight", f"{p}.bn1"))
                o = F.relu(conv(o, f"{p}.conv2.weight", f"{p}.bn2", stride, 1))
                o = conv(o, f"{p}.conv3.weight", f"{p}.bn3")
            else:
                o = F.relu(conv(x, f"{p}.conv1.weight", f"{p}.bn1", stride, 1))
                o = conv(o, f"{p}.conv2.weight", f"{p}.bn2", 1, 1)
            if f"{p}.downsample.0.weight" in sd:
                idn = conv(x, f"{p}.downsample.0.weight", f"{p}.downsample.1", stride, 0)
            x = F.relu(o + idn)
    return F.linear(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1), sd["fc.weight"], sd["fc.bias"])


def head30_model(num_layers, modalities):
    """The realistic-magnitude networks: trained-looking BatchNorm, head x 30 (|logit| about 4.7 for ResNet-50 6-ch, 11 for ResNet-152 12-ch)."""
    from types import SimpleNamespace

    from salve_amd import synthetic
    from salve_amd.models.early_fusion import EarlyFusionCEResnet

    torch.manual_seed(0)
    model = EarlyFusionCEResnet(num_layers, False, 2, SimpleNamespace(modalities=modalities))
    synthetic.trained_looking_batchnorm(model)
    synthetic.trained_looking_head(model, 30.0)
    return model.eval()


HEAD30_CASES = [(50, ["floor_rgb_texture"], 4, 4.5), (152, ["ceiling_rgb_texture", "floor_rgb_texture"], 2, 9.0)]   # layers, modalities, batch, least |logit|


def default_bn_case():
    """ResNet-152, one surface, torch's default BatchNorm statistics (activations ~1e8), batch 2: (model, inputs)."""
    from types import SimpleNamespace

    from salve_amd.models.early_fusion import EarlyFusionCEResnet

    torch.manual_seed(0)
    model = EarlyFusionCEResnet(152, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    return model, tile_like_inputs(2, 2, seed=2)
