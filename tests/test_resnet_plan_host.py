"""The verifier's launch plan without a GPU: salve_amd/csrc/resnet_plan.h compiled for the host as a stand-alone program
(tests/host/resnet_plan_host.cpp), once with -O2 and once under AddressSanitizer and UBSan, run as a child process on the op programs of
every network the product builds, on the programs of tests/verifier_cases.py and on every prefix of ResNet-50's.

The logits are bit-identical whichever kernels run, so no GPU test can tell a wrong plan that still computes; here the plans are pinned:
tests/golden/resnet_plans.json holds the steps of every full program at flags 0 and at each single flag, as the commit BEFORE the planner
decided them (its decision code, read by its forward pass's own walk over the ops, printed these strings; that code and the planner
agreed on every program and prefix here at all 8192 flag values: profiles/r23_resnet_plan.txt)."""

import json
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import verifier_cases as vc
from salve_amd import _lib
from salve_amd.models import hip_resnet, resnet_factory
from salve_amd.models.early_fusion import EarlyFusionCEResnet

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "resnet_plans.json"

FLAGS = {name[len("RESNET_"):]: getattr(_lib, name) for name in dir(_lib) if name.startswith("RESNET_") and isinstance(getattr(_lib, name), int)}
ALL_FLAGS = sum(FLAGS.values())
MODALITIES = {6: ["floor_rgb_texture"], 12: ["ceiling_rgb_texture", "floor_rgb_texture"], 18: ["ceiling_rgb_texture", "floor_rgb_texture", "layout"]}
LAYERS = (18, 34, 50, 101, 152)

# token -> the ops its step consumes
COUNT = {"stem": 2, "block": 3, "block_proj": 3, "block_next": 4, "block_next_even": 4, "conv": 1, "conv8": 1, "conv8_auto": 1, "maxpool": 1, "fc": 1,
         "x128": 1, "x256": 1, "x256_split": 1, "x128_w16": 1, "c128_128": 2, "c128_256": 2, "c256_256": 2, "c128_256_split": 2, "c256_256_split": 2,
         "c128_128_w16": 2, "c128_256_even": 2, "c128_256_split_even": 2}


def test_the_flag_table_is_the_abi_s():
    assert len(FLAGS) == 13 and ALL_FLAGS == 8191 and sorted(FLAGS.values()) == [1 << k for k in range(13)]


# ---------------------------------------------------------------------------------------------------- the programs
def network_program(layers, channels):
    torch.manual_seed(layers * 100 + channels)
    # (the model factory has no 101-layer branch, as the reference's has none; the op builder has: ResNet-50's model around a 101-layer trunk)
    model = EarlyFusionCEResnet(50 if layers == 101 else layers, False, 2, SimpleNamespace(modalities=MODALITIES[channels]))
    if layers == 101:
        model.resnet = resnet_factory.ResNetTrunk(101)
    ops, _, _, ktab, cin_p = hip_resnet.build_program(model.state_dict(), layers, (224, 224))
    assert cin_p == {6: 8, 12: 16, 18: 24}[channels]
    return ops, ktab


def full_programs():
    """{name: (ops, ktab)}: the fifteen networks at 224 x 224, and the block / chain / stem programs at the shapes of test_gpu_verifier_ops.py."""
    progs = {f"resnet{layers}-{ch}ch": network_program(layers, ch) for layers in LAYERS for ch in (6, 12, 18)}
    for h, w in vc.BLOCK_SIZES:
        progs[f"block-{h}x{w}"] = vc.pack(vc.block_program(h, w, vc.BLOCK_BATCHES[0]).bld)[::3]
    for mid, midn, b, h, w in vc.CHAIN_CASES:
        progs[f"chain-{mid}-{midn}-{h}x{w}"] = vc.pack(vc.chain_program(mid, midn, b, h, w).bld)[::3]
    for cin, h, b in vc.STEM_POOL_CASES:
        progs[f"stem-{cin}-{h}x224"] = vc.pack(vc.stem_program(cin, h, b).bld)[::3]
    return progs


def write_input(path, programs):
    """[(ops, ktab, [flags], [(flags, op, batch)])] -> the file tests/host/resnet_plan_host.cpp reads."""
    with open(path, "wb") as f:
        f.write(np.int32(len(programs)).tobytes())
        for ops, ktab, flags, queries in programs:
            assert ops.dtype == hip_resnet.OP_DTYPE
            f.write(np.array([len(ops), len(ktab), len(flags), len(queries)], dtype=np.int32).tobytes())
            f.write(ops.tobytes())
            f.write(np.ascontiguousarray(ktab, dtype=np.int32).tobytes())
            f.write(np.array(flags, dtype=np.int32).tobytes())
            f.write(np.array(queries, dtype=np.int32).reshape(-1).tobytes())


def wide_threshold_batch(o):
    """The smallest batch at which ceil(M / 256) * (Cout / 256) reaches 1536 tiles, M = batch * Ho * Wo."""
    hw, nt = int(o["Ho"]) * int(o["Wo"]), int(o["Cout"]) // 256
    m_tiles = -(-1536 // nt)                      # ceil(M / 256) >= m_tiles  <=>  M > (m_tiles - 1) * 256
    b = (m_tiles - 1) * 256 // hw + 1
    tiles = lambda batch: -(-batch * hw // 256) * nt
    assert tiles(b - 1) < 1536 <= tiles(b)
    return b


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    work = tmp_path_factory.mktemp("resnet_plan_host")
    src = str(ROOT / "tests" / "host" / "resnet_plan_host.cpp")
    builds = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
    for name, opts in builds.items():
        subprocess.run(["g++", "-std=c++17", *opts, "-o", str(work / name), src], check=True)

    def run(programs):
        """-> ({(program index, flags): [tokens] or "REFUSED message"}, {(program index, flags, op, batch): answer}); both builds must
        end with status 0 and print the same."""
        write_input(work / "in.bin", programs)
        outs = []
        for name in builds:
            done = subprocess.run([str(work / name), str(work / "in.bin")], capture_output=True, text=True)
            assert done.returncode == 0, (name, done.stderr[-4000:])
            outs.append(done.stdout)
        assert outs[0] == outs[1]
        plans, answers = {}, {}
        for line in outs[0].splitlines():
            head, _, rest = line.partition(":")
            kind, *nums = head.split()
            if kind == "P":
                plans[int(nums[0]), int(nums[2])] = rest.strip() if rest.startswith(" REFUSED") else rest.split()
            else:
                answers[tuple(int(v) for v in nums)] = int(rest)
        return plans, answers

    return run


@pytest.fixture(scope="module")
def programs():
    return full_programs()


@pytest.fixture(scope="module")
def plans(planner, programs):
    """{program name: {flag name ("0" for none): [tokens]}} of the full programs."""
    flag_list = [0] + sorted(FLAGS.values())
    got, _ = planner([(ops, ktab, flag_list, []) for ops, ktab in programs.values()])
    names = {0: "0", **{v: k for k, v in FLAGS.items()}}
    return {prog: {names[f]: got[i, f] for f in flag_list} for i, prog in enumerate(programs)}


def covered(tokens, n_ops):
    """The steps cover ops 0 .. n_ops - 1 exactly once, in order, and every token consumes the count its name says."""
    at = 0
    for t in tokens:
        span, _, name = t.partition(":")
        first, count = (int(v) for v in span.split("+"))
        assert first == at and count == COUNT[name], (t, at)
        at += count
    return at == n_ops


def names_of(tokens):
    return [t.partition(":")[2] for t in tokens]


# ---------------------------------------------------------------------------------------------------- the tests
def test_every_plan_covers_its_program(plans, programs):
    assert len(programs) == 15 + len(vc.BLOCK_SIZES) + len(vc.CHAIN_CASES) + len(vc.STEM_POOL_CASES)
    for prog, by_flag in plans.items():
        for flag, tokens in by_flag.items():
            assert isinstance(tokens, list) and covered(tokens, len(programs[prog][0])), (prog, flag)


def test_the_plans_are_the_recorded_ones(plans):
    want = json.loads(GOLDEN.read_text())
    assert sorted(want) == sorted(plans)
    for prog, by_flag in plans.items():
        assert sorted(want[prog]) == sorted(by_flag), prog
        for flag, tokens in by_flag.items():
            assert " ".join(tokens) == want[prog][flag], (prog, flag)


def test_the_default_plan_uses_every_step_kind_and_form(plans):
    seen = {n for by_flag in plans.values() for n in names_of(by_flag["0"])}
    assert seen == {"stem", "block", "block_proj", "block_next_even", "block_next", "conv", "conv8_auto", "fc", "x128", "x256_split",
                    "c128_128", "c128_256_split", "c128_256_split_even", "c256_256_split"}
    assert all(names_of(by_flag["NO_STEM_FUSE"])[:2] == ["conv", "maxpool"] for prog, by_flag in plans.items() if prog[:5] in ("resne", "stem-"))
    r50 = names_of(plans["resnet50-6ch"]["0"])
    assert r50[:5] == ["stem", "block_proj", "block", "block_next_even", "conv"] and r50[-1] == "fc"
    # layer 2: blocks 1 and 2 chained, block 3 into layer 3 with Y's even pixels; layer 3: blocks 1 .. 4 chained, block 5 alone (no (256, 512) form)
    assert r50.count("c128_128") == 2 and r50.count("c128_256_split_even") == 1 and r50.count("c256_256_split") == 4 and r50.count("x256_split") == 1
    assert len(r50) == 36
    assert set(names_of(plans["resnet18-6ch"]["0"])) == {"stem", "conv", "conv8_auto", "fc"}     # BasicBlock networks: nothing to fuse behind the stem


def test_each_flag_removes_exactly_its_own_steps(plans):
    for prog, by_flag in plans.items():
        base = names_of(by_flag["0"])
        n = {flag: names_of(tokens) for flag, tokens in by_flag.items()}
        blocks = lambda names: [t for t in names if t.startswith("block")]
        chains = lambda names: [t for t in names if t[0] in "xc" and t[1].isdigit()]
        assert "stem" not in n["NO_STEM_FUSE"] and blocks(n["NO_STEM_FUSE"]) == blocks(base) and chains(n["NO_STEM_FUSE"]) == chains(base), prog
        assert not blocks(n["NO_BLOCK_FUSE"]) and n["NO_BLOCK_FUSE"].count("stem") == base.count("stem"), prog
        assert "block_proj" not in n["NO_PROJ_FUSE"] and [t for t in blocks(n["NO_PROJ_FUSE"])] == [t for t in blocks(base) if t != "block_proj"], prog
        assert not [t for t in n["NO_NEXT_FUSE"] if t.startswith("block_next")], prog
        assert [t.replace("_next_even", "").replace("_next", "") for t in blocks(base)] == blocks(n["NO_NEXT_FUSE"]), prog
        assert not chains(n["NO_CHAIN"]) and blocks(n["NO_CHAIN"]) == blocks(base), prog
        assert not [t for t in n["CHAIN_EXPAND_ONLY"] if t.startswith("c") and t[1].isdigit()], prog
        assert len(chains(n["CHAIN_EXPAND_ONLY"])) == len(chains(base)) and blocks(n["CHAIN_EXPAND_ONLY"]) == blocks(base), prog
        assert not [t for t in n["CHAIN_STORE_ALL"] if t.endswith("_even")] and [t.replace("_even", "") for t in base] == n["CHAIN_STORE_ALL"], prog
        assert not [t for t in n["CONV_IGEMM_ONLY"] if t.startswith("conv8")] and [t.replace("conv8_auto", "conv") for t in base] == n["CONV_IGEMM_ONLY"], prog
        assert "conv8_auto" not in n["CONV8_WHEREVER"] and [t for t in n["CONV8_WHEREVER"] if not t.startswith("conv")] == [t for t in base if not t.startswith("conv")], prog
        # the 16-wave / 256-pixel-tile forms exist for the all-128-channel shapes only, the channel-split forms for the 256-channel ones
        w16 = {"x128": "x128_w16", "c128_128": "c128_128_w16"}
        assert n["CHAIN_16_WAVES"] == [w16.get(t, t) for t in base] and not [t for t in base if t.endswith("_w16")], prog
        assert n["CHAIN_NO_SPLIT"] == [t.replace("_split", "") for t in base] and not {"x256", "c128_256", "c128_256_even", "c256_256"} & set(base), prog
        assert by_flag["ROUND_ROBIN_TILES"] == by_flag["0"] == by_flag["NO_TRANSPOSED_TILES"], prog     # launch arguments, not the plan


def test_every_prefix_of_resnet50_plans_within_its_ops(planner, programs):
    """A planner that looks at ops[i + 1] .. ops[i + 3] past the end of a program reads outside the heap block the ops are in: the
    sanitized build ends with an error (`planner` asserts its exit status)."""
    ops, ktab = programs["resnet50-6ch"]
    flag_list = [0] + sorted(FLAGS.values()) + [ALL_FLAGS]
    got, _ = planner([(ops[:n].copy(), ktab, flag_list, []) for n in range(1, len(ops) + 1)])
    assert len(got) == len(ops) * len(flag_list)
    for (i, flag), tokens in got.items():
        assert covered(tokens, i + 1), (i + 1, flag)
    whole = got[len(ops) - 1, 0]
    for i in range(len(ops) - 1):          # a prefix that ends at a step boundary of the whole plan may only differ in its last steps' even-pixel stores
        cut = [t for t in whole if int(t.split("+")[0]) + COUNT[t.partition(":")[2]] <= i + 1]
        if sum(COUNT[t.partition(":")[2]] for t in cut) == i + 1:
            assert [t.replace("_even", "") for t in got[i, 0]] == [t.replace("_even", "") for t in cut], i + 1


REFUSALS = [
    (dict(op=7), "unknown op"),
    (dict(Cout=96), "conv: Cout must be a multiple of 64"),
    (dict(Cin=60), "conv: Cin must be a multiple of 8"),
    (dict(Cin=8), "conv: KH*KW*Cin must be a multiple of 64"),
    (dict(in2_buf=0, Cin2=64, stride2=1, Hi2=8, Wi2=8, KH=3, KW=3, pad=1), "conv: a second source needs a 1x1 / stride 1 / pad 0 convolution without residual"),
    (dict(in2_buf=0, Cin2=64, stride2=1, Hi2=8, Wi2=8, stride=2), "conv: a second source needs a 1x1 / stride 1 / pad 0 convolution without residual"),
    (dict(in2_buf=0, Cin2=64, stride2=1, Hi2=8, Wi2=8, res_buf=0), "conv: a second source needs a 1x1 / stride 1 / pad 0 convolution without residual"),
    (dict(in2_buf=0, Cin2=0, stride2=1, Hi2=8, Wi2=8), "conv: bad second-source geometry"),
    (dict(in2_buf=0, Cin2=72, stride2=1, Hi2=8, Wi2=8), "conv: bad second-source geometry"),
    (dict(in2_buf=0, Cin2=64, stride2=0, Hi2=8, Wi2=8), "conv: bad second-source geometry"),
    (dict(in2_buf=0, Cin2=64, stride2=2, Hi2=8, Wi2=15), "conv: bad second-source geometry"),
    (dict(in2_buf=0, Cin2=64, stride2=2, Hi2=15, Wi2=17), "conv: bad second-source geometry"),
    (dict(op=hip_resnet.OP_MAXPOOL, Cin=60), "maxpool: C must be a multiple of 8"),
    (dict(op=hip_resnet.OP_AVGPOOL_FC, Cout=0), "fc: 1..8 classes supported"),
    (dict(op=hip_resnet.OP_AVGPOOL_FC, Cout=9), "fc: 1..8 classes supported"),
    (dict(op=hip_resnet.OP_AVGPOOL_FC, Cout=2, Cin=60), "fc: C must be a multiple of 8"),
]


def test_the_refusals_and_their_messages(planner):
    """One good op (a 1x1 convolution 64 -> 64 at 8 x 8, buffer 0 -> 1) and that op with one field wrong, as the LAST of three ops: the
    message is check_op's, whatever the flags."""
    good = np.zeros(1, dtype=hip_resnet.OP_DTYPE)
    for k, v in dict(op=hip_resnet.OP_CONV, in_buf=0, out_buf=1, res_buf=hip_resnet.NO_BUF, Hi=8, Wi=8, Cin=64, Ho=8, Wo=8, Cout=64, KH=1, KW=1, stride=1,
                     pad=0, relu=1, in2_buf=hip_resnet.NO_BUF).items():
        good[k] = v
    cases = []
    for fields, _ in REFUSALS:
        bad = good.copy()
        for k, v in fields.items():
            bad[k] = v
        cases.append((np.concatenate([good, good, bad]), np.zeros(8, np.int32), [0, ALL_FLAGS], []))
    got, _ = planner([(np.concatenate([good, good, good]), np.zeros(8, np.int32), [0, ALL_FLAGS], [])] + cases)
    assert got[0, 0] == ["0+1:conv", "1+1:conv", "2+1:conv"] == got[0, ALL_FLAGS]
    for i, (_, message) in enumerate(REFUSALS):
        assert got[i + 1, 0] == got[i + 1, ALL_FLAGS] == "REFUSED " + message, (i, got[i + 1, 0])


def test_the_batch_dependent_choice_flips_at_1536_tiles(planner, programs, plans):
    """ResNet-50's 14 x 14 convolutions into 1024 channels.  The first block of layer 3 ends in one with the projection shortcut in its k
    (K = 256 + 512): the 8-phase kernel under the automatic mode, so conv_igemm_kernel below 1536 tiles of 256 x 256 and the 8-phase
    kernel from there on -- batch 500 | 501.  The others (K = 256, not compute-bound) are expand-chain steps, or under NO_CHAIN plain
    convolutions that never take the 8-phase kernel by default; with CONV8_WHEREVER every one of them takes it at any batch."""
    ops, ktab = programs["resnet50-6ch"]
    expand = [i for i, o in enumerate(ops) if o["op"] == hip_resnet.OP_CONV and (o["Ho"], o["Wo"], o["Cout"], o["KH"]) == (14, 14, 1024, 1)]
    assert len(expand) == 6
    auto = [i for i in expand if f"{i}+1:conv8_auto" in plans["resnet50-6ch"]["0"]]
    assert auto == expand[:1] and ops[auto[0]]["in2_buf"] != hip_resnet.NO_BUF
    hi = wide_threshold_batch(ops[auto[0]])
    assert hi == 501
    no_chain, wherever = FLAGS["NO_CHAIN"], FLAGS["NO_CHAIN"] | FLAGS["CONV8_WHEREVER"]
    queries = [(f, i, b) for f in (0, no_chain, wherever) for i in expand for b in (1, hi - 1, hi, 4096)]
    _, answers = planner([(ops, ktab, [], queries)])
    for f, i, b in queries:
        if f == wherever:
            want = 1
        elif i == auto[0]:
            want = int(b >= hi)
        else:
            want = -1 if f == 0 else 0          # flags 0: no CONV step starts there (an expand-chain step does)
        assert answers[0, f, i, b] == want, (f, i, b)
