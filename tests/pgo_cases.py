"""Cases for salve_pose_graph_optimise and a float64 emulator of include/salve_hip.h's statement of it (pose-graph optimisation: the
reference's `--method pgo`, salve/algorithms/pose2_slam.py:57-286).  The emulator shares no code with the library.  It keeps the header's
order of every sum -- the cost's 256 partial sums folded by halving, a block's rows in row order, the right-looking Cholesky -- so what
separates it from the device is the last place of sin / cos / atan2 and nothing else.  Besides the outputs it returns, for every decision
that depends on a rounded value (Huber's n <= k, the wrap, accept, the two stop tests), the RELATIVE distance of the deciding quantity from
its threshold (`margins`): check_conditions() asks that no shipped case decides closer than MIN_MARGIN, with the library's own trigonometry
and with every sin / cos / atan2 result nudged by an ulp, so that the integer outputs can be compared exactly on the device.
(lambda's own arithmetic -- x 10, / 10, > 1e5 -- has no rounded input: it is the same IEEE sequence on both sides and carries no margin.  An
accept of E(x + d) = E(x) = 0 carries none either: it is reached by exact zeros only.)

The tolerances and max_iterations are arguments of the entry, and most cases here stop at a chosen iteration cap or at tolerances looser
than gtsam's 1e-5: a Gauss-Newton run to 1e-5 usually ends with a step whose decrease is 1e-9 of the cost or less, which is no decision a
test could pin.  The minimum itself is pinned in tests/test_pgo_cases_host.py, against scipy, at tolerances of 1e-14.

Measured there (python -m pytest tests/test_pgo_cases_host.py -k independent_minimiser -s, scipy 1.15, which prints every floor's figure):
the largest pose difference between the emulator's minimum and scipy.optimize.least_squares' over all cases is D0_MEASURED = 5.415e-7 (floor 53
of the 70-floor launch, two Huber-weighted factors and a smallest eigenvalue of 0.03; the plain least-squares floors stay below 1.2e-7); the
test asserts 4 x that.  It is scipy's own error -- a finite-difference Jacobian -- not the emulator's: the device is compared with the emulator.
"""

import math
from functools import lru_cache

import numpy as np

ROW = np.dtype([("i1", "<i4"), ("i2", "<i4"), ("prob", "<f4"), ("y_hat", "<i4"), ("R", "<f4", (4,)), ("t", "<f4", (2,)), ("s", "<f8")])
NODE_OUT = np.dtype([("localized", "<i4"), ("parent", "<i4"), ("depth", "<i4"), ("reserved", "<i4"), ("R", "<f4", (4,)), ("t", "<f4", (2,)), ("s", "<f8")])
PGO_FLOOR_OUT = np.dtype([("n_unknown_nodes", "<i4"), ("n_factors", "<i4"), ("n_iterations", "<i4"), ("n_rejected", "<i4"), ("n_downweighted", "<i4"),
                          ("stop_reason", "<i4"), ("lambda", "<f8"), ("cost_initial", "<f8"), ("cost_final", "<f8")])
assert ROW.itemsize == 48 and NODE_OUT.itemsize == 48 and PGO_FLOOR_OUT.itemsize == 48
GUARD, SENTINEL = 3, 0xA5
LDS_NODES = 56            # SALVE_PGO_LDS_NODES
STOP_EMPTY, STOP_ABSOLUTE, STOP_RELATIVE, STOP_LAMBDA, STOP_MAX_ITERATIONS, STOP_NON_FINITE = 0, 1, 2, 3, 4, 5
PI, TWO_PI = 3.141592653589793, 6.283185307179586
LAMBDA_INITIAL, LAMBDA_FACTOR, LAMBDA_UPPER = 1e-5, 10.0, 1e5
QNAN = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), dtype="<f8")[0]
MIN_MARGIN = 1e-6
NUDGE_BOUND = 1e-11       # how far an ulp on every sin / cos / atan2 may move an output
D0_MEASURED = 5.415e-7    # see the module docstring
DEFAULTS = {"robust": 1, "huber_k": 1.345, "odometry_sigmas": (0.2, 0.2, 0.1), "prior_sigmas": (0.3, 0.3, 0.1), "max_iterations": 100,
            "relative_error_tol": 1e-5, "absolute_error_tol": 1e-5, "confidence_threshold": 0.5}


# ---- trigonometry: the library's, or every result an ulp off

class Trig:
    cos, sin, atan2 = staticmethod(math.cos), staticmethod(math.sin), staticmethod(math.atan2)


class NudgedTrig:
    """Every result moved by one ulp, up or down by a fixed pseudo-random sequence."""

    def __init__(self, seed):
        self.state = seed * 2654435761 % 2 ** 32

    def _nudge(self, v):
        self.state = (1103515245 * self.state + 12345) % 2 ** 31
        return math.nextafter(v, math.inf if (self.state >> 16) & 1 else -math.inf)

    def cos(self, a): return self._nudge(math.cos(a))
    def sin(self, a): return self._nudge(math.sin(a))
    def atan2(self, y, x): return self._nudge(math.atan2(y, x))


# ---- the emulator of one floor

def _empty_floor(n, raised):
    nodes = np.zeros(n, dtype=NODE_OUT)
    nodes["parent"], nodes["depth"] = -1, -1
    fo = np.zeros(1, dtype=PGO_FLOOR_OUT)
    fo["lambda"], fo["cost_initial"], fo["cost_final"] = LAMBDA_INITIAL, QNAN, QNAN
    return {"nodes": nodes, "pose": np.full((n, 3), QNAN), "floor": fo[0], "raised": raised, "margins": []}


def emulate_floor(rows, n, init, P, trig=Trig, variant=None):
    """One VERIFIED floor (its rows keep the row contract, 0 <= n <= max_nodes, every parent in [-1, n)): `rows` its ROW records, `init` its n
    NODE_OUT records, P the arguments (DEFAULTS' keys).  variant: None, or the name of an emulated WRONG kernel (WRONG_KERNELS)."""
    margins = []
    localized = [bool(init["localized"][v]) for v in range(n)]
    if not any(localized):
        return _empty_floor(n, False)
    origin = localized.index(True)
    idx, k = [-1] * n, 0
    for v in range(n):
        if localized[v]:
            idx[v], k = k, k + 1
    L, N = k, 3 * k
    sig_o, sig_p = [float(s) for s in P["odometry_sigmas"]], [float(s) for s in P["prior_sigmas"]]
    if variant == "sigmas-swapped":
        sig_o, sig_p = sig_p, sig_o
    hk, robust = float(P["huber_k"]), int(P["robust"])
    thr = np.float32(P["confidence_threshold"])

    def wrap(a):
        if variant == "no-wrap":
            return a
        w = a - TWO_PI * math.ceil((a - PI) / TWO_PI)
        margins.append(("wrap", (PI - abs(w)) / PI))
        return w

    def pose_of(x, y, th):
        return [x, y, th, trig.cos(th), trig.sin(th)]

    X, nonfinite = {}, False
    for v in range(n):
        if localized[v]:
            r = init[v]
            th = trig.atan2(float(r["R"][2]), float(r["R"][0]))
            X[v] = pose_of(float(r["t"][0]), float(r["t"][1]), th)
            nonfinite |= not math.isfinite(((X[v][0] + X[v][1]) + float(r["R"][0])) + float(r["R"][2]))

    candidate = lambda r: r["y_hat"] == 1 and (r["prob"] > thr if variant == "threshold-gt" else r["prob"] >= thr)
    factors, extra = [], 0   # (position in the floor, i1, i2, measurement)
    for q, r in enumerate(rows):
        if not candidate(r):
            continue
        a, b = int(r["i1"]), int(r["i2"])
        if idx[a] < 0 or idx[b] < 0:
            extra += variant == "unlocalized-not-skipped"
            continue
        nonfinite |= not math.isfinite(((float(r["t"][0]) + float(r["t"][1])) + float(r["R"][0])) + float(r["R"][2]))
        th = trig.atan2(float(r["R"][2]), float(r["R"][0]))
        factors.append((q, a, b, (float(r["t"][0]), float(r["t"][1]), th, trig.cos(th), trig.sin(th)), float(r["prob"])))
    if variant == "best-row-only":
        best = {}
        for f in factors:
            if (f[1], f[2]) not in best or f[4] > best[(f[1], f[2])][4]:
                best[(f[1], f[2])] = f
        factors = sorted(best.values())

    fo = np.zeros(1, dtype=PGO_FLOOR_OUT)[0]
    fo["n_unknown_nodes"], fo["n_factors"] = L, (0 if variant == "no-prior" else 1) + len(factors) + extra
    fo["lambda"], fo["cost_initial"], fo["cost_final"] = LAMBDA_INITIAL, QNAN, QNAN

    def weigh(r):
        ss = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
        nn = math.sqrt(ss)
        if robust and math.isfinite(nn):
            margins.append(("huber", abs(nn - hk) / hk))
        if robust and nn > hk:
            rho, w, down = hk * (nn - 0.5 * hk), hk / nn, 1
        else:
            rho, w, down = 0.5 * ss, 1.0, 0
        sw = math.sqrt(w)
        return [sw * r[0], sw * r[1], sw * r[2]], rho, sw, down

    def between(X1, X2, m, jac):
        if variant == "measurement-swapped":
            X1, X2 = X2, X1
        vx, vy = X1[0] - X2[0], X1[1] - X2[1]
        dx, dy = X2[3] * vx + X2[4] * vy, X2[3] * vy - X2[4] * vx
        ux, uy = dx - m[0], dy - m[1]
        r = [(m[3] * ux + m[4] * uy) / sig_o[0], (m[3] * uy - m[4] * ux) / sig_o[1], wrap((X1[2] - X2[2]) - m[2]) / sig_o[2]]
        rs, rho, sw, down = weigh(r)
        if not jac:
            return rs, rho, down, None, None
        cd, sd = X1[3] * X2[3] + X1[4] * X2[4], X1[4] * X2[3] - X1[3] * X2[4]
        ce, se = m[3] * cd + m[4] * sd, m[3] * sd - m[4] * cd
        sj = 1.0 if variant == "huber-on-residual-only" else sw
        a0, a1, a2 = sj / sig_o[0], sj / sig_o[1], sj / sig_o[2]
        J1 = [[a0 * ce, a0 * -se, 0.0], [a1 * se, a1 * ce, 0.0], [0.0, 0.0, a2]]
        J2 = [[a0 * -m[3], a0 * -m[4], a0 * (m[3] * dy - m[4] * dx)], [a1 * m[4], a1 * -m[3], a1 * (-(m[4] * dy) - m[3] * dx)], [0.0, 0.0, -a2]]
        if variant == "measurement-swapped":
            J1, J2 = J2, J1
        return rs, rho, down, J1, J2

    def prior(Xo, jac):
        r = [Xo[0] / sig_p[0], Xo[1] / sig_p[1], wrap(Xo[2]) / sig_p[2]]
        rs, rho, sw, down = weigh(r)
        if not jac:
            return rs, rho, down, None
        sj = 1.0 if variant == "huber-on-residual-only" else sw
        a0, a1, a2 = sj / sig_p[0], sj / sig_p[1], sj / sig_p[2]
        return rs, rho, down, [[a0 * Xo[3], a0 * -Xo[4], 0.0], [a1 * Xo[4], a1 * Xo[3], 0.0], [0.0, 0.0, a2]]

    def cost(Xc):
        partial, down = [0.0] * 256, 0
        if variant != "no-prior":
            _, partial[0], down, _ = prior(Xc[origin], False)
        for q, a, b, m, _ in factors:
            _, rho, d, _, _ = between(Xc[a], Xc[b], m, False)
            partial[q % 256] += rho
            down += d
        h = 128
        while h >= 1:
            for t in range(h):
                partial[t] += partial[t + h]
            h //= 2
        return partial[0], down

    def add_JtJ(H, u, w, A, B):
        for p in range(3):
            for q in range(3):
                H[u + p, w + q] += (A[0][p] * B[0][q] + A[1][p] * B[1][q]) + A[2][p] * B[2][q]

    def add_Jtr(gs, u, A, r):
        for p in range(3):
            gs[u + p] += (A[0][p] * r[0] + A[1][p] * r[1]) + A[2][p] * r[2]

    def linearise(Xc):
        H, gs = np.zeros((N, N)), np.zeros(N)
        if variant != "no-prior":
            rs, _, _, J = prior(Xc[origin], True)
            add_JtJ(H, 3 * idx[origin], 3 * idx[origin], J, J)
            add_Jtr(gs, 3 * idx[origin], J, rs)
        for q, a, b, m, _ in factors:   # (row order: every block's and every segment's own order)
            rs, _, _, J1, J2 = between(Xc[a], Xc[b], m, True)
            ua, ub = 3 * idx[a], 3 * idx[b]
            add_JtJ(H, ub, ua, J2, J1)
            add_JtJ(H, ua, ua, J1, J1)
            add_JtJ(H, ub, ub, J2, J2)
            add_Jtr(gs, ua, J1, rs)
            add_Jtr(gs, ub, J2, rs)
        return H, -gs

    def solve(H, g, lam):
        """(H + lam I) d = g on the lower triangle: right-looking Cholesky, column by column, then the two substitutions.  None: a bad pivot."""
        A, y = H.copy(), g.copy()
        A[np.arange(N), np.arange(N)] += lam
        with np.errstate(all="ignore"):
            for j in range(N):
                piv = A[j, j]
                if not (piv > 0.0 and math.isfinite(piv)):
                    return None
                ljj = math.sqrt(piv)
                A[j + 1:, j] = A[j + 1:, j] / ljj
                A[j, j] = ljj
                col = A[j + 1:, j]
                A[j + 1:, j + 1:] -= col[:, None] * col[None, :]   # (the strict upper part is never read)
            for j in range(N):
                yj = y[j] / A[j, j]
                y[j + 1:] -= A[j + 1:, j] * yj
                y[j] = yj
            for j in range(N - 1, -1, -1):
                dj = y[j] / A[j, j]
                y[:j] -= A[j, :j] * dj
                y[j] = dj
        return y

    lam, stop, iterations, rejected, trace = LAMBDA_INITIAL, 0, 0, 0, []
    if nonfinite:
        stop = STOP_NON_FINITE
    else:
        E, down = cost(X)
        fo["n_downweighted"], fo["cost_initial"], fo["cost_final"] = down, E, E
        while not stop:
            if iterations >= int(P["max_iterations"]):
                stop = STOP_MAX_ITERATIONS
                break
            iterations += 1
            H, g = linearise(X)
            carried = 0.0
            while True:
                d = solve(H, g, lam + carried)
                accepted = False
                if d is not None:
                    XT = dict(X)
                    for v in X:
                        u, Xv = 3 * idx[v], X[v]
                        XT[v] = pose_of(Xv[0] + (Xv[3] * d[u] - Xv[4] * d[u + 1]), Xv[1] + (Xv[4] * d[u] + Xv[3] * d[u + 1]), Xv[2] + d[u + 2])
                    En, down_n = cost(XT)
                    accepted = math.isfinite(En) and En <= E
                    trace.append((E, En, lam, accepted))
                    if math.isfinite(En) and math.isfinite(E) and not (En == 0.0 and E == 0.0):
                        margins.append(("accept", abs(En - E) / max(abs(E), abs(En))))
                    if variant == "stop-on-absolute-decrease" and not accepted and math.isfinite(En) and \
                            (abs(E - En) <= P["absolute_error_tol"] or (E > 0 and abs(E - En) / E <= P["relative_error_tol"])):
                        stop = STOP_ABSOLUTE
                        break
                if accepted:
                    break
                rejected += 1
                if variant == "lambda-not-restored":
                    carried += lam   # (the damping of the rejected attempt stays on the diagonal)
                lam *= LAMBDA_FACTOR
                if lam > LAMBDA_UPPER:
                    stop = STOP_LAMBDA
                    break
            if stop:
                break
            decrease, E_old = E - En, E
            X, E = XT, En
            fo["cost_final"], fo["n_downweighted"] = E, down_n
            lam /= LAMBDA_FACTOR
            margins.append(("absolute", abs(decrease - P["absolute_error_tol"]) / P["absolute_error_tol"]))
            if decrease <= P["absolute_error_tol"]:
                stop = STOP_ABSOLUTE
            else:
                margins.append(("relative", abs(decrease / E_old - P["relative_error_tol"]) / P["relative_error_tol"]))
                if decrease / E_old <= P["relative_error_tol"]:
                    stop = STOP_RELATIVE
    fo["n_iterations"], fo["n_rejected"], fo["stop_reason"], fo["lambda"] = iterations, rejected, stop, lam

    out = _empty_floor(n, False)
    for v in X:
        o = out["nodes"][v]
        o["localized"], o["parent"], o["depth"] = 1, init["parent"][v], init["depth"][v]
        o["R"] = np.array([X[v][3], -X[v][4], X[v][4], X[v][3]]).astype(np.float32)
        o["t"], o["s"] = np.array(X[v][:2]).astype(np.float32), 1.0
        out["pose"][v] = X[v][:3]
    out["floor"], out["margins"], out["trace"] = fo, margins, trace   # trace: (E, E(x + d), lambda, accepted) of every solved attempt
    return out


WRONG_KERNELS = ("best-row-only", "no-prior", "no-wrap", "huber-on-residual-only", "lambda-not-restored", "measurement-swapped",
                 "unlocalized-not-skipped", "threshold-gt", "sigmas-swapped", "stop-on-absolute-decrease")


# ---- the launch: the tables verified as the kernel verifies them, floor by floor

def params(case, **override):
    P = dict(DEFAULTS)
    P.update(case.get("params", {}))
    P.update(override)
    return P


def floor_is_malformed(case, f):
    rows, fs, M = case["rows"], case["floor_start"], case["max_nodes"]
    lo, hi, n = int(fs[f]), int(fs[f + 1]), int(case["n_nodes"][f])
    if lo < 0 or hi < lo or hi > len(rows) or n < 0 or n > M:
        return True
    r = rows[lo:hi]
    if ((r["i1"] < 0) | (r["i1"] >= r["i2"]) | (r["i2"] >= n)).any():
        return True
    key = r["i1"].astype(np.int64) * 65536 + r["i2"]
    if (np.diff(key) < 0).any():
        return True
    parent = case["init"][f * M:f * M + n]["parent"]
    return bool(((parent < -1) | (parent >= n)).any())


def emulate(case, trig=Trig, variant=None, **override):
    """Per floor of the launch: emulate_floor's dict (a malformed floor: empty, raised)."""
    P, M, out = params(case, **override), case["max_nodes"], []
    for f in range(len(case["n_nodes"])):
        n = int(case["n_nodes"][f])
        if floor_is_malformed(case, f):
            out.append(_empty_floor(min(max(n, 0), M) if 0 <= n <= M else 0, True))
            continue
        lo, hi = int(case["floor_start"][f]), int(case["floor_start"][f + 1])
        out.append(emulate_floor(case["rows"][lo:hi], n, case["init"][f * M:f * M + n], P, trig, variant))
    return out


_EXPECTED = {}


def expected(name):
    """(the emulator's per-floor results of the shipped case, computed once and left unchanged)"""
    if name not in _EXPECTED:
        _EXPECTED[name] = emulate(case(name))
    return _EXPECTED[name]


def fresh_buffers(c):
    """(out_nodes, out_pose, out_floors) as sentinel-filled host arrays with GUARD records in front and behind"""
    F, M = len(c["n_nodes"]), c["max_nodes"]
    mk = lambda count, dt: np.frombuffer(bytes([SENTINEL]) * ((count + 2 * GUARD) * dt.itemsize), dtype=dt).copy()
    return mk(F * M, NODE_OUT), mk(F * M, np.dtype(("<f8", (3,)))), mk(F, PGO_FLOOR_OUT)


def expected_buffers(c, results):
    """fresh_buffers with the emulator's results written where the entry writes: a floor's first n_nodes records, nothing else."""
    nodes, pose, floors = fresh_buffers(c)
    M = c["max_nodes"]
    for f, res in enumerate(results):
        n = len(res["nodes"])
        nodes[GUARD + f * M:GUARD + f * M + n] = res["nodes"]
        pose[GUARD + f * M:GUARD + f * M + n] = res["pose"]
        floors[GUARD + f] = res["floor"]
    return nodes, pose, floors


# ---- building cases

def make_rows(entries):
    """entries: (i1, i2, prob, y_hat, (x, y, theta)[, scale]) -> ROW records, stably sorted by (i1, i2)"""
    rows = np.zeros(len(entries), dtype=ROW)
    for r, e in zip(rows, entries):
        x, y, th = e[4]
        r["i1"], r["i2"], r["prob"], r["y_hat"] = e[0], e[1], e[2], e[3]
        r["R"], r["t"], r["s"] = [math.cos(th), -math.sin(th), math.sin(th), math.cos(th)], [x, y], (e[5] if len(e) > 5 else 1.0)
    return rows[np.lexsort((rows["i2"], rows["i1"]))] if len(rows) else rows


def make_init(n, poses, M=None):
    """poses: {node: (x, y, theta)} -> NODE_OUT [M or n]; a chain for a tree (parent: the previous localized node)"""
    init = np.zeros(M or n, dtype=NODE_OUT)
    init["parent"], init["depth"] = -1, -1
    prev, depth = -1, 0
    for v in sorted(poses):
        x, y, th = poses[v]
        o = init[v]
        o["localized"], o["parent"], o["depth"] = 1, prev, depth
        o["R"], o["t"], o["s"] = [math.cos(th), -math.sin(th), math.sin(th), math.cos(th)], [x, y], 1.0
        prev, depth = v, depth + 1
    return init


def relative(pb, pa):
    """m = x_b^-1 x_a: the measurement of BetweenFactorPose2(X(b), X(a), m)"""
    vx, vy, c, s = pa[0] - pb[0], pa[1] - pb[1], math.cos(pb[2]), math.sin(pb[2])
    return (c * vx + s * vy, c * vy - s * vx, pa[2] - pb[2])


def one_floor(name, n, entries, poses, M=None, **P):
    rows = make_rows(entries)
    return {"name": name, "rows": rows, "floor_start": np.array([0, len(rows)], dtype=np.int32), "n_nodes": np.array([n], dtype=np.int32),
            "max_nodes": M or n, "init": make_init(n, poses, M), "params": P}


def noisy_floor(name, n, seed, extra_edges, noise=(0.03, 0.02), init_noise=(0.2, 0.1), M=None, ring=False, outliers=0, **P):
    """n panoramas on a walk; measurements between neighbours (and `extra_edges` random pairs) with noise; the initial poses off by init_noise."""
    rs = np.random.RandomState(seed)
    truth, p = {}, np.zeros(3)
    for v in range(n):
        truth[v] = tuple(p)
        if ring:
            ang = 2 * math.pi * (v + 1) / n
            p = np.array([40 * math.cos(ang) - 40, 40 * math.sin(ang), ang])
        else:
            p = p + np.array([2.0 * math.cos(p[2]), 2.0 * math.sin(p[2]), rs.uniform(-0.9, 0.9)])
    pairs = [(v, v + 1) for v in range(n - 1)] + ([(0, n - 1)] if ring else [])
    while len(pairs) < n - 1 + extra_edges + bool(ring):
        a, b = sorted(rs.choice(n, 2, replace=False))
        pairs.append((int(a), int(b)))
    entries = []
    for k, (a, b) in enumerate(pairs):
        m = np.array(relative(truth[b], truth[a])) + rs.normal(0, 1, 3) * [noise[0], noise[0], noise[1]]
        if k >= len(pairs) - outliers:
            m = m + [1.5, -1.0, 0.8]
        entries.append((a, b, 0.9, 1, tuple(m)))
    poses = {v: tuple(np.array(truth[v]) + (rs.normal(0, 1, 3) * [init_noise[0], init_noise[0], init_noise[1]] if v else 0)) for v in range(n)}
    c = one_floor(name, n, entries, poses, M, **P)
    c["truth"] = truth
    return c


def launch_of(name, floors, M, **P):
    """Several one-floor cases as ONE launch of max_nodes M (their own params are dropped: a launch has one set)."""
    rows = np.concatenate([f["rows"] for f in floors])
    init = np.zeros(len(floors) * M, dtype=NODE_OUT)
    init["parent"], init["depth"] = -1, -1
    for k, f in enumerate(floors):
        n = int(f["n_nodes"][0])
        init[k * M:k * M + min(n, M)] = f["init"][:min(n, M)]
    return {"name": name, "rows": rows, "floor_start": np.concatenate([[0], np.cumsum([len(f["rows"]) for f in floors])]).astype(np.int32),
            "n_nodes": np.array([f["n_nodes"][0] for f in floors], dtype=np.int32), "max_nodes": M, "init": init, "params": P}


def single_floor_launch(c, f):
    """Floor f of a launch as a launch of its own over the SAME row table (so a malformed extent stays what it is)."""
    M = c["max_nodes"]
    return {"name": f"{c['name']}[{f}]", "rows": c["rows"], "floor_start": c["floor_start"][f:f + 2].copy(), "n_nodes": c["n_nodes"][f:f + 1].copy(),
            "max_nodes": M, "init": c["init"][f * M:(f + 1) * M].copy(), "params": c["params"]}


H = math.pi / 2
# the reference's own recorded case (tests/algorithms/test_pose2_slam.py::test_planar_slam_pgo_only): six slots, pose 0 unknown, robust off
REFERENCE_INIT = {1: (0.5, 0.0, 0.2), 2: (2.3, 0.1, -0.2), 3: (4.1, 0.1, H), 4: (4.0, 2.0, math.pi), 5: (2.1, 2.1, -H)}
REFERENCE_MEASUREMENTS = [(1, 2, (-2.0, 0.0, 0.0)), (2, 3, (0.0, 2.0, -H)), (3, 4, (0.0, 2.0, -H)), (4, 5, (0.0, 2.0, -H)), (2, 5, (2.0, 0.0, H))]
REFERENCE_EXPECTED = {1: (0.0, 0.0, 0.0), 2: (2.0, 0.0, 0.0), 3: (4.0, 0.0, H), 4: (4.0, 2.0, math.pi), 5: (2.0, 2.0, -H)}


@lru_cache(maxsize=None)
def _cases():
    out = []
    out.append(one_floor("reference-recorded", 6, [(a, b, 0.99, 1, m) for a, b, m in REFERENCE_MEASUREMENTS], REFERENCE_INIT, robust=0,
                         max_iterations=5))
    out.append(one_floor("two-nodes-zero-residual", 2, [(0, 1, 0.9, 1, (-1.0, 0.0, 0.0), 1.7)], {0: (0.0, 0.0, 0.0), 1: (1.0, 0.0, 0.0)}))
    tri_truth = {0: (0.0, 0.0, 0.0), 1: (2.0, 0.0, 0.7), 2: (1.0, 1.5, -0.4)}
    tri = [(0, 1, 0.9, 1, relative(tri_truth[1], tri_truth[0])), (1, 2, 0.9, 1, relative(tri_truth[2], tri_truth[1])),
           (0, 2, 0.9, 1, tuple(np.array(relative(tri_truth[2], tri_truth[0])) + [0.9, -0.6, 0.35]))]
    tri_init = {0: (0.0, 0.0, 0.0), 1: (2.1, -0.1, 0.75), 2: (0.9, 1.6, -0.45)}
    out.append(one_floor("triangle-huber", 3, tri, tri_init, max_iterations=6))
    out.append(one_floor("triangle-huber-robust-off", 3, tri, tri_init, robust=0, max_iterations=3))
    # two and three candidate rows on a pair that disagree; rows that must not count: below the threshold, y_hat == 0, a NaN prob; one AT the threshold
    sq = {0: (0.0, 0.0, 0.0), 1: (2.0, 0.0, H), 2: (2.0, 2.0, math.pi - 0.2), 3: (0.0, 2.0, -H)}
    rel = lambda a, b, off=(0, 0, 0): tuple(np.array(relative(sq[b], sq[a])) + off)
    out.append(one_floor("several-rows-per-pair", 4, [
        (0, 1, 0.95, 1, rel(0, 1, (0.05, 0.0, 0.02))), (0, 1, 0.99, 1, rel(0, 1, (-0.08, 0.03, -0.03))),
        (1, 2, 0.9, 1, rel(1, 2)), (1, 2, 0.8, 1, rel(1, 2, (0.1, 0.1, 0.05))), (1, 2, 0.85, 1, rel(1, 2, (-0.05, 0.12, -0.06))),
        (2, 3, 0.75, 1, rel(2, 3, (0.02, -0.02, 0.01))), (2, 3, 0.7499, 1, rel(2, 3, (3.0, 3.0, 1.0))), (2, 3, 0.99, 0, rel(2, 3, (-3.0, 2.0, -1.0))),
        (0, 3, float("nan"), 1, rel(0, 3, (2.0, 2.0, 2.0))), (0, 3, 0.97, 1, rel(0, 3, (0.04, 0.04, -0.02))),
        (0, 2, 0.6, 1, rel(0, 2, (5.0, 5.0, 1.0)))],
        {0: (0.0, 0.0, 0.0), 1: (2.1, 0.1, H + 0.05), 2: (1.9, 2.1, math.pi - 0.25), 3: (0.1, 1.9, -H - 0.05)}, confidence_threshold=0.75, max_iterations=2))
    # poses at theta = +-pi, measurements across the branch cut
    bc = {0: (0.0, 0.0, 0.0), 1: (-2.0, 0.1, math.pi - 0.05), 2: (-4.0, 0.0, -math.pi + 0.05)}
    out.append(one_floor("branch-cut", 3, [(0, 1, 0.9, 1, relative(bc[1], bc[0])), (1, 2, 0.9, 1, relative(bc[2], bc[1])),
                                           (0, 2, 0.9, 1, tuple(np.array(relative(bc[2], bc[0])) + [0.05, 0.02, -0.03]))],
                         {0: (0.0, 0.0, 0.0), 1: (-2.1, 0.15, -math.pi - 0.02), 2: (-3.9, 0.05, math.pi + 0.1)}, max_iterations=2))
    # a second component whose nodes stay unlocalized, rows that touch them, an origin that is not compact index 0
    comp = {2: (0.0, 0.0, 0.0), 3: (1.5, 0.5, 0.3), 5: (3.0, -0.5, -0.6), 6: (4.0, 1.0, 1.0)}
    crel = lambda a, b, off=(0, 0, 0): tuple(np.array(relative(comp[b], comp[a])) + off)
    out.append(one_floor("second-component", 8, [
        (0, 1, 0.9, 1, (1.0, 0.0, 0.1)), (0, 2, 0.9, 1, (9.0, 9.0, 1.0)), (1, 5, 0.9, 1, (-7.0, 3.0, 2.0)), (2, 3, 0.9, 1, crel(2, 3, (0.03, 0.0, 0.01))),
        (3, 5, 0.9, 1, crel(3, 5, (0.0, -0.04, 0.02))), (5, 6, 0.9, 1, crel(5, 6)), (2, 6, 0.9, 1, crel(2, 6, (0.05, 0.05, -0.02))), (6, 7, 0.9, 1, (2.0, 2.0, 0.5)),
        (4, 7, 0.9, 1, (1.0, 1.0, 0.0))],
        {2: (0.3, -0.2, 0.1), 3: (1.6, 0.4, 0.35), 5: (3.1, -0.4, -0.5), 6: (3.9, 1.1, 0.9)}, max_iterations=4))
    # an initial estimate far off: the emulator rejects steps (check_conditions asserts n_rejected > 0)
    far = noisy_floor("far-off-start", 7, seed=3, extra_edges=5, init_noise=(3.0, 2.5), max_iterations=8)
    out.append(far)
    # the same start with a tolerance of 28: its three rejected steps RAISE the cost by 27.3, 26.6 and 19.6, the first accepted ones lower it by
    # 31.1, 112.9, 100.6, 68.5 and 14.9 -- a stop test on |decrease| of a rejected step would end it at once
    out.append(noisy_floor("rejected-steps-inside-the-tolerance", 7, seed=3, extra_edges=5, init_noise=(3.0, 2.5), absolute_error_tol=28.0,
                           relative_error_tol=1e-12))
    out.append(noisy_floor("stops-at-the-iteration-cap", 9, seed=5, extra_edges=6, max_iterations=2))
    out.append(noisy_floor("stops-at-absolute-tol", 9, seed=6, extra_edges=6, absolute_error_tol=1e-2, relative_error_tol=1e-12))
    out.append(noisy_floor("stops-at-relative-tol", 9, seed=7, extra_edges=6, outliers=2, absolute_error_tol=1e-12, relative_error_tol=3e-3))
    # every pivot overflows (sigma 1e-160, a zero residual): eleven rejections to the lambda bound, the poses as they went in
    out.append(one_floor("stops-at-the-lambda-bound", 2, [(0, 1, 0.9, 1, (-1.0, 0.0, 0.0))], {0: (0.0, 0.0, 0.0), 1: (1.0, 0.0, 0.0)}, robust=0,
                         odometry_sigmas=(1e-160,) * 3, prior_sigmas=(1e-160,) * 3))
    # both sides of the LDS / workspace switch (SALVE_PGO_LDS_NODES localized nodes), one exactly at it
    for L in (LDS_NODES - 1, LDS_NODES, LDS_NODES + 1):
        out.append(noisy_floor(f"{L}-nodes", L, seed=L, extra_edges=L, M=64, max_iterations=3))
    out.append(noisy_floor("256-node-ring", 256, seed=11, extra_edges=0, noise=(0.01, 0.002), init_noise=(0.05, 0.01), ring=True, max_iterations=3))
    nf = one_floor("non-finite-measurement", 3, tri, tri_init)
    nf["rows"]["t"][1, 0] = np.inf
    out.append(nf)
    # 70 floors of mixed sizes in one launch: an edgeless floor, a lone localized node, one of each malformed kind
    floors = [noisy_floor(f"f{k}", 3 + (k * 7) % 11, seed=100 + k, extra_edges=k % 5, outliers=k % 2) for k in range(66)]
    floors[5] = noisy_floor("f5", LDS_NODES + 2, seed=105, extra_edges=20, M=None)
    floors[9] = one_floor("edgeless", 3, [], {})
    floors[12] = one_floor("lone-node", 2, [], {1: (0.5, 0.5, 0.5)})
    bad_row = noisy_floor("bad-row", 5, seed=201, extra_edges=2)
    bad_row["rows"]["i2"][2] = 5
    unsorted = noisy_floor("unsorted", 5, seed=202, extra_edges=2)
    unsorted["rows"] = unsorted["rows"][::-1].copy()
    bad_parent = noisy_floor("bad-parent", 5, seed=203, extra_edges=2)
    bad_parent["init"]["parent"][3] = 5
    too_many = noisy_floor("too-many-nodes", 4, seed=204, extra_edges=1)
    floors += [bad_row, unsorted, bad_parent, too_many]
    launch = launch_of("70-floors", floors, 64, max_iterations=2)
    launch["n_nodes"][69] = 65                    # n_nodes > max_nodes
    launch["floor_start"][31] = -1                # a bad extent: floors 30 (hi < lo) and 31 (lo < 0)
    out.append(launch)
    return tuple(out)


def cases():
    return list(_cases())


def case(name):
    return next(c for c in _cases() if c["name"] == name)


MALFORMED_70 = (30, 31, 66, 67, 68, 69)
EXACT_ZERO_CASES = ("two-nodes-zero-residual", "stops-at-the-lambda-bound")


def check_conditions(names=None):
    """The conditions on the INPUTS that let the device's integers be compared exactly: no decision within MIN_MARGIN of its threshold, with
    the library's trigonometry and with every result an ulp off; under that nudge the outputs move by at most NUDGE_BOUND and no count changes."""
    for c in cases():
        if names is not None and c["name"] not in names:
            continue
        base = expected(c["name"])
        # (a case of exact zeros -- sin 0 = 0, cos 0 = 1, atan2(0, 1) = 0 in every library -- is not nudged: an ulp would make it another case)
        nudged = base if c["name"] in EXACT_ZERO_CASES else emulate(c, trig=NudgedTrig(len(c["name"])))
        for f, (a, b) in enumerate(zip(base, nudged)):
            for res in (a, b):
                worst = min(res["margins"], key=lambda m: m[1], default=("none", 1.0))
                assert worst[1] >= MIN_MARGIN, (c["name"], f, worst)
            assert a["floor"].tobytes()[:24] == b["floor"].tobytes()[:24] and a["raised"] == b["raised"], (c["name"], f)
            assert np.array_equal(np.isnan(a["pose"]), np.isnan(b["pose"]))
            if np.isfinite(a["pose"]).any():
                assert np.nanmax(np.abs(a["pose"] - b["pose"])) <= NUDGE_BOUND, (c["name"], f, np.nanmax(np.abs(a["pose"] - b["pose"])))
            for k in ("cost_initial", "cost_final"):
                if np.isfinite(a["floor"][k]):
                    assert abs(a["floor"][k] - b["floor"][k]) <= NUDGE_BOUND * max(1.0, abs(a["floor"][k])), (c["name"], f, k)
    assert expected("far-off-start")[0]["floor"]["n_rejected"] > 0
    stops = {n: int(expected(n)[0]["floor"]["stop_reason"]) for n in ("stops-at-the-iteration-cap", "stops-at-absolute-tol", "stops-at-relative-tol",
                                                                       "stops-at-the-lambda-bound", "non-finite-measurement", "two-nodes-zero-residual")}
    assert list(stops.values()) == [STOP_MAX_ITERATIONS, STOP_ABSOLUTE, STOP_RELATIVE, STOP_LAMBDA, STOP_NON_FINITE, STOP_ABSOLUTE], stops
    assert expected("256-node-ring")[0]["floor"]["n_iterations"] <= 10
    assert [f for f, r in enumerate(expected("70-floors")) if r["raised"]] == list(MALFORMED_70)


# ---- the floor of tests/test_gpu_pose_graph_pgo_floor.py: ten panoramas of a truth, measured twice per neighbour pair and over loops

FLOOR_SEED = 6
# Chosen on the CPU (python -c "from tests import pgo_cases as pc, floor_report_cases as fc; from pathlib import Path;
# print(pc.floor_cpu_errors(fc.golden_1210(Path('tests/golden'))[1]))"): the mean distance of the panoramas from the truth, the estimate laid on
# the truth by its origin panorama, of the spanning tree and of the optimised poses (the emulators of tests/pose_graph_cases.py and of this
# file), in the truth's coordinates.  The GPU test asserts the report's own figure (a RANSAC alignment) the same way round.
FLOOR_TREE_ERR, FLOOR_PGO_ERR = 0.2365, 0.0661


def floor_measurements(truth, seed=FLOOR_SEED):
    """(i1, i2, prob, y_hat, y_true, (x, y, theta)) per prediction, in file order: the chain of the first ten panoramas with a confident and a
    less confident noisy hypothesis per pair, six loop closures, and three confident FALSE positives next to a true hypothesis of their pair."""
    rng = np.random.default_rng(seed)
    ids = [int(p) for p in truth.pano_ids[:10]]
    pose = {int(p): (float(truth.t[k][0]), float(truth.t[k][1]), math.atan2(float(truth.R[k][1, 0]), float(truth.R[k][0, 0]))) for k, p in enumerate(truth.pano_ids)}
    noisy = lambda a, b, st, sr: tuple(np.array(relative(pose[b], pose[a])) + rng.normal(0, 1, 3) * [st, st, sr])
    out = []
    for k in range(9):
        a, b = sorted((ids[k], ids[k + 1]))
        out.append((a, b, 0.99, 1, 1, noisy(a, b, 0.12, 0.08)))
        out.append((a, b, 0.9, 1, 1, noisy(a, b, 0.03, 0.02)))
    for ka, kb in ((0, 4), (3, 8), (0, 9), (2, 6), (5, 9), (1, 7)):
        a, b = sorted((ids[ka], ids[kb]))
        out.append((a, b, 0.95, 1, 1, noisy(a, b, 0.03, 0.02)))
    for k in (1, 4, 7):
        a, b = sorted((ids[k], ids[k + 1]))
        out.append((a, b, 0.97, 1, 0, tuple(np.array(relative(pose[b], pose[a])) + [0.8, -0.6, 0.9])))
    out.append((sorted((ids[2], ids[3]))[0], sorted((ids[2], ids[3]))[1], 0.3, 1, 1, noisy(*sorted((ids[2], ids[3])), 0.03, 0.02)))   # below the threshold
    out.append((sorted((ids[6], ids[7]))[0], sorted((ids[6], ids[7]))[1], 0.99, 0, 0, (3.0, 3.0, 1.0)))                                # predicted a mismatch
    return out, pose


def floor_cpu_errors(truth):
    """(tree, pgo): see FLOOR_TREE_ERR"""
    from tests import pose_graph_cases as tree_cases

    meas, pose = floor_measurements(truth)
    ids = sorted({m[0] for m in meas} | {m[1] for m in meas})
    rows = make_rows([(ids.index(a), ids.index(b), prob, y_hat, m) for a, b, prob, y_hat, _, m in meas])
    node_out = tree_cases.emulate_floor(rows, len(ids), 0.5, 0.5, 0.01, 0)[1]
    init = np.zeros(len(ids), dtype=NODE_OUT)
    for k in init.dtype.names:
        init[k] = node_out[k]
    res = emulate_floor(rows, len(ids), init, dict(DEFAULTS))
    origin = pose[ids[int(np.nonzero(init["localized"])[0][0])]]
    c, s = math.cos(origin[2]), math.sin(origin[2])
    errs = []
    for est in (np.stack([init["t"][:, 0], init["t"][:, 1]], 1).astype(np.float64), res["pose"][:, :2]):
        world = np.stack([c * est[:, 0] - s * est[:, 1] + origin[0], s * est[:, 0] + c * est[:, 1] + origin[1]], 1)
        loc = init["localized"] == 1
        errs.append(float(np.mean(np.linalg.norm(world[loc] - np.array([pose[i][:2] for i in ids])[loc], axis=1))))
    return errs[0], errs[1], res["floor"]
