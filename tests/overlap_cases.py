"""salve_bev_pair_overlap (include/salve_hip.h): a numpy emulator of the entry, the case list the host and the GPU tests share, and
emulated WRONG kernels (every mistake the kernel's alignment peeling, reduction and row store invite) that the case list must catch.

A case is a dict: name, h, w, bev_a / bev_b (uint32 [STACK, h, w]; `bev_b is bev_a` for the same-array cases), a_index / b_index (int64 [n_jobs])
and bad (does a job name an image outside its array).  Image stacks hold STACK = 5 images, so that with a 16-byte aligned array and an odd
h * w the start residues 0, 4, 8 and 12 bytes mod 16 all occur, for a and b independently.  `run_case(case, fn)` hands `fn` an output buffer
filled with SENTINEL, GUARD rows on both sides, and returns (whole buffer, status bit raised)."""

from __future__ import annotations

import numpy as np

GEOMETRIES = [(1, 1), (1, 5), (3, 7), (16, 16), (17, 31), (63, 65), (64, 64), (501, 501)]
JOB_COUNTS = [0, 1, 63, 64, 65, 257]
STACK = 5
SENTINEL = -7777777
GUARD = 3
COLOUR_BITS = 0x00FFFFFF
STATUS_BAD_TILE_JOB = 16   # include/salve_hip.h: SALVE_STATUS_BAD_TILE_JOB

WRONG_KERNELS = ("top_byte_counted", "red_byte_only", "tail_pixels_dropped", "head_pixels_dropped", "head_read_from_neighbour", "union_is_a_plus_b",
                 "one_residue_for_both", "last_partial_wave_lost", "row_written_to_next", "row_written_to_previous", "bad_job_unwritten",
                 "counts_16_bit")


def head_pixels(index: int, hw: int) -> int:
    """Pixels of image `index` in front of its first 16-byte boundary, in a 16-byte aligned array of images of hw pixels."""
    return ((16 - (index * hw * 4) % 16) % 16) // 4


def emulate(bev_a: np.ndarray, bev_b: np.ndarray, h: int, w: int, a_index, b_index, out: np.ndarray, wrong: str = None) -> bool:
    """Rows [0, n_jobs) of `out` (int32 [n_jobs, 4], or a view with room around it for the wrong kernels that miss their row) as
    salve_bev_pair_overlap writes them; returns whether the bad-job status bit is raised.  wrong: one of WRONG_KERNELS."""
    hw = h * w
    fa = np.ascontiguousarray(bev_a).view(np.uint32).reshape(-1)
    fb = np.ascontiguousarray(bev_b).view(np.uint32).reshape(-1)
    bits = {"top_byte_counted": 0xFFFFFFFF, "red_byte_only": 0xFF}.get(wrong, COLOUR_BITS)
    occ_a, occ_b = (fa & np.uint32(bits)) != 0, (fb & np.uint32(bits)) != 0
    n_a, n_b = fa.size // hw, fb.size // hw
    raised = False
    px = np.arange(hw)
    for j, (ia, ib) in enumerate(zip(np.asarray(a_index).tolist(), np.asarray(b_index).tolist())):
        row = j + {"row_written_to_next": 1, "row_written_to_previous": -1}.get(wrong, 0)
        if not (0 <= ia < n_a and 0 <= ib < n_b):
            raised = True
            if wrong != "bad_job_unwritten":
                out[row] = -1
            continue
        ha, hb = head_pixels(ia, hw), head_pixels(ib, hw)
        oa, ob = occ_a[ia * hw:(ia + 1) * hw], occ_b[ib * hw:(ib + 1) * hw]
        if wrong == "head_read_from_neighbour":   # every image read from the 16-byte boundary BELOW its start
            back_a, back_b = (4 - ha) % 4, (4 - hb) % 4
            oa, ob = occ_a[ia * hw - back_a:(ia + 1) * hw - back_a], occ_b[ib * hw - back_b:(ib + 1) * hw - back_b]
        if wrong == "one_residue_for_both" and ha != hb:   # b's aligned chunks paired with a's without the shift between the two grids
            shifted = np.zeros(hw, dtype=bool)
            src = px + (hb - ha)
            ok = (src >= 0) & (src < hw)
            shifted[ok] = ob[src[ok]]
            ob = shifted
        keep = np.ones(hw, dtype=bool)
        if wrong == "tail_pixels_dropped":
            keep &= px < ha + (hw - ha) // 4 * 4
        if wrong == "head_pixels_dropped":
            keep &= px >= ha
        if wrong == "last_partial_wave_lost":   # 64 chunks of 4 pixels per wave step
            keep &= px < hw // 256 * 256
        oa, ob = oa & keep, ob & keep
        inter, na, nb = int((oa & ob).sum()), int(oa.sum()), int(ob.sum())
        union = na + nb if wrong == "union_is_a_plus_b" else int((oa | ob).sum())
        vals = np.array([inter, union, na, nb], dtype=np.int64)
        if wrong == "counts_16_bit":
            vals &= 0xFFFF
        out[row] = vals.astype(np.int32)
    return raised


def run_case(case, fn):
    """(int32 [GUARD + n_jobs + GUARD, 4] as `fn(case, out_rows)` left it, the status bit `fn` reports).  fn writes rows of the view it is given."""
    n = len(case["a_index"])
    buf = np.full((GUARD + n + GUARD, 4), SENTINEL, dtype=np.int32)
    raised = fn(case, buf)
    return buf, bool(raised)


def emulated(wrong: str = None):
    """`run_case`'s fn for the emulator (or one of its wrong kernels)."""
    def fn(case, buf):
        n = len(case["a_index"])
        # a view whose index -1 is the guard row in front (numpy would wrap -1 to the end): rows shifted by hand
        class Rows:
            def __setitem__(self, r, v):
                buf[GUARD + r] = v
        return emulate(case["bev_a"], case["bev_b"], case["h"], case["w"], case["a_index"], case["b_index"], Rows(), wrong)
    return fn


def _random_stack(rng, h, w, densities):
    out = np.zeros((STACK, h, w), dtype=np.uint32)
    for k, p in enumerate(densities):
        colour = rng.integers(1, 1 << 24, size=(h, w), dtype=np.uint32)
        out[k] = np.where(rng.random((h, w)) < p, colour, 0)
    return out


def _all_pairs():
    a, b = np.meshgrid(np.arange(STACK), np.arange(STACK), indexing="ij")
    return a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)


def make_cases():
    cases = []

    def add(name, h, w, bev_a, bev_b, a_index, b_index):
        a_index, b_index = np.asarray(a_index, dtype=np.int64), np.asarray(b_index, dtype=np.int64)
        bad = bool(((a_index < 0) | (a_index >= STACK) | (b_index < 0) | (b_index >= STACK)).any())
        cases.append({"name": f"{h}x{w}-{name}", "h": h, "w": w, "bev_a": bev_a, "bev_b": bev_b, "a_index": a_index, "b_index": b_index, "bad": bad})

    pa, pb = _all_pairs()
    for gi, (h, w) in enumerate(GEOMETRIES):
        rng = np.random.default_rng(100 + gi)
        zeros = np.zeros((STACK, h, w), dtype=np.uint32)
        add("empty", h, w, zeros, zeros.copy(), pa, pb)
        full = rng.integers(1, 1 << 24, size=(STACK, h, w), dtype=np.uint32)
        add("full", h, w, full, full[::-1].copy(), pa, pb)
        left, right = full.copy(), full.copy()
        flat_l, flat_r = left.reshape(STACK, -1), right.reshape(STACK, -1)
        flat_l[:, (h * w) // 2:] = 0     # disjoint halves of the pixel run (a 1 x 1 image: a empty, b full)
        flat_r[:, :(h * w) // 2] = 0
        add("disjoint-halves", h, w, left, right, pa, pb)
        ra = _random_stack(rng, h, w, [0.01, 0.5, 0.99, 0.5, 0.01])
        rb = _random_stack(rng, h, w, [0.5, 0.99, 0.01, 0.01, 0.99])
        add("random", h, w, ra, rb, pa, pb)
        # single-byte contents: only the red byte's lowest bit, only the blue byte's, only the (unoccupied) top byte, and mixtures
        pick = rng.integers(0, 4, size=(STACK, h, w))
        values = np.array([0, 0x00000001, 0x00010000, 0xFF000000], dtype=np.uint32)
        by = np.stack([np.where(pick[0] == 1, values[1], 0), np.where(pick[1] == 2, values[2], 0), np.where(pick[2] == 3, values[3], 0),
                       values[pick[3]], values[pick[4]] | np.where(pick[3] == 3, np.uint32(0xFF000000), np.uint32(0))]).astype(np.uint32)
        by[0].reshape(-1)[-1] = 0x00000001   # the last pixel, the first pixel and the lone top byte always occur
        by[1].reshape(-1)[0] = 0x00010000
        by[2].reshape(-1)[0] = 0xFF000000
        add("single-bytes", h, w, by, by[::-1].copy(), pa, pb)
        add("same-array", h, w, ra, ra, np.r_[np.arange(STACK), pa], np.r_[np.arange(STACK), pb])
        perm = rng.permutation(pa.shape[0])
        add("permuted", h, w, ra, rb, pa[perm], pb[perm])
        add("bad-jobs", h, w, ra, rb, [0, STACK, 1, -1, 2, 3, 2 ** 31 - 1, 4, -2 ** 31, 2], [1, 0, -1, 2, STACK, 3, 0, 2 ** 31 - 1, 4, 4])
        add("all-bad", h, w, ra, rb, [STACK, -1], [0, STACK + 7])
    # job counts on one odd geometry (and the largest once): many jobs sharing one b
    for h, w, counts in ((17, 31, JOB_COUNTS), (501, 501, [65])):
        rng = np.random.default_rng(7 * h)
        ra = _random_stack(rng, h, w, [0.3, 0.6, 0.9, 0.1, 0.5])
        rb = _random_stack(rng, h, w, [0.5, 0.2, 0.8, 0.4, 0.7])
        for n in counts:
            add(f"{n}-jobs-one-b", h, w, ra, rb, rng.integers(0, STACK, size=n), np.full(n, 3))
            add(f"{n}-jobs", h, w, ra, rb, rng.integers(0, STACK, size=n), rng.integers(0, STACK, size=n))
    return cases


_CASES = None


def cases():
    """The case list, built once and shared (nothing may write to its arrays)."""
    global _CASES
    if _CASES is None:
        _CASES = make_cases()
        for c in _CASES:
            for k in ("bev_a", "bev_b", "a_index", "b_index"):
                c[k].setflags(write=False)
    return _CASES


_EXPECTED = {}


def expected(case):
    """(buffer, status bit) of the emulator for `case`, computed once."""
    if case["name"] not in _EXPECTED:
        _EXPECTED[case["name"]] = run_case(case, emulated())
    return _EXPECTED[case["name"]]
