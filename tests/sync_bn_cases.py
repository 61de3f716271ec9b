"""The synchronised BatchNorm (salve_bn_*_stats -> salve_bn_combine -> salve_bn_*_apply, salve_bn_*_backward_reduce ->
salve_bn_*_backward_apply; include/salve_hip.h) restated in float64 numpy, pass by pass, for the host tests (which hold it against
full-batch BatchNorm) and the GPU tests (which hold the kernels against it).  Not a test module.

`split_forward` / `split_backward` run the chain over a list of row counts, one per emulated rank; `wrong=` swaps one pass for a
plausible wrong kernel (WRONG), which the cases must tell from the right one."""

import numpy as np

RELU, ADD = 1, 2
WRONG = ("biased_running_var", "averaged_means", "local_rows", "no_relu_mask", "empty_rank_not_skipped")
# row splits of 1, 2, 3 and 5 ranks: unequal shards, a rank with 0 rows (first, in the middle, last) and a rank with 1 row
SPLITS = ((12,), (7, 5), (1, 11), (0, 9, 3), (5, 0, 7), (4, 1, 7), (3, 0, 1, 6, 2), (2, 5, 1, 4, 0))


def make_case(rows, c, seed, flags=0):
    """x, residual, dy [rows, c], gamma, beta, running_mean, running_var [c] in float64; channel means far from zero and of
    different scales, so that a mean of means or a biased variance is visibly wrong."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.5, 3.0, c)
    x = rng.standard_normal((rows, c)) * scale + rng.uniform(-4.0, 4.0, c) + np.linspace(0.0, 2.0, rows)[:, None]   # (a drift along the rows)
    return dict(x=x, residual=rng.standard_normal((rows, c)), dy=rng.standard_normal((rows, c)), gamma=rng.uniform(0.5, 1.5, c),
                beta=rng.uniform(-0.5, 0.5, c), running_mean=rng.standard_normal(c), running_var=rng.uniform(0.5, 2.0, c), flags=flags,
                eps=1e-5, momentum=0.1)


# ---- full-batch BatchNorm (torch's definitions), the thing the chain must equal -------------------------------------------------
def full_forward(case):
    x, n = case["x"], case["x"].shape[0]
    mean, var = x.mean(axis=0), x.var(axis=0)
    invstd = 1.0 / np.sqrt(var + case["eps"])
    m = case["momentum"]
    rm = (1 - m) * case["running_mean"] + m * mean
    rv = (1 - m) * case["running_var"] + m * var * n / (n - 1)
    y = (x - mean) * invstd * case["gamma"] + case["beta"]
    if case["flags"] & ADD:
        y = y + case["residual"]
    if case["flags"] & RELU:
        y = np.maximum(y, 0.0)
    return dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv)


def full_backward(case, fwd):
    x, n = case["x"], case["x"].shape[0]
    g = np.where(fwd["y"] > 0, case["dy"], 0.0) if case["flags"] & RELU else case["dy"]
    xhat = (x - fwd["mean"]) * fwd["invstd"]
    dbeta, dgamma = g.sum(axis=0), (g * xhat).sum(axis=0)
    dx = case["gamma"] * fwd["invstd"] * (g - dbeta / n - xhat * dgamma / n)
    return dict(dx=dx, dres=g if case["flags"] & ADD else None, dgamma=dgamma, dbeta=dbeta)


# ---- the passes ------------------------------------------------------------------------------------------------------------------
def stats(x):
    """salve_bn_*_stats: [2, C] = mean, M2 of the rows; zeros without rows."""
    if x.shape[0] == 0:
        return np.zeros((2, x.shape[1]))
    mean = x.mean(axis=0)
    return np.stack([mean, ((x - mean) ** 2).sum(axis=0)])


def combine(partials, rows, eps, momentum, running_mean, running_var, wrong=None):
    """salve_bn_combine: Chan's formula in rank order, ranks without rows skipped -> mean, invstd, running_mean, running_var."""
    c = partials[0].shape[1]
    total = int(sum(rows))
    if wrong == "averaged_means":   # every rank weighs the same, the spread between the ranks' means is lost
        live = [p for p, n in zip(partials, rows) if n]
        m, q = np.mean([p[0] for p in live], axis=0), np.sum([p[1] for p in live], axis=0)
    else:
        n, m, q = 0.0, np.zeros(c), np.zeros(c)
        for p, nb in zip(partials, rows):
            if nb == 0 and wrong != "empty_rank_not_skipped":
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                f = np.float64(nb) / np.float64(n + nb)   # (0 / 0 where an empty rank comes first and is not skipped)
            d = p[0] - m
            m = m + d * f
            q = q + p[1] + d * d * (n * f)
            n += nb
    var = q / total
    unbiased = var if wrong == "biased_running_var" else q / (total - 1)
    return m, 1.0 / np.sqrt(var + eps), (1 - momentum) * running_mean + momentum * m, (1 - momentum) * running_var + momentum * unbiased


def apply(x, residual, gamma, beta, mean, invstd, flags):
    """salve_bn_*_apply."""
    y = (x - mean) * (gamma * invstd) + beta
    if flags & ADD:
        y = y + residual
    return np.maximum(y, 0.0) if flags & RELU else y


def backward_reduce(dy, x, y, mean, invstd, flags, wrong=None):
    """salve_bn_*_backward_reduce: [2, C] = sum g, sum g * xhat over the rows."""
    g = np.where(y > 0, dy, 0.0) if (flags & RELU and wrong != "no_relu_mask") else dy
    return np.stack([g.sum(axis=0), (g * (x - mean) * invstd).sum(axis=0)])


def backward_apply(dy, x, y, gamma, mean, invstd, sums, total_rows, flags, wrong=None):
    """salve_bn_*_backward_apply: the ranks' sums [world, 2, C] added in rank order -> dx, dres."""
    g = np.where(y > 0, dy, 0.0) if flags & RELU else dy
    s = sums[0].copy()
    for r in range(1, len(sums)):
        s = s + sums[r]
    n = max(x.shape[0], 1) if wrong == "local_rows" else total_rows
    dx = gamma * invstd * (g - s[0] / n - (x - mean) * invstd * s[1] / n)
    return dx, (g if flags & ADD else None)


# ---- the chain over emulated ranks -----------------------------------------------------------------------------------------------
def bounds(rows):
    hi = np.cumsum(rows)
    return list(zip((hi - rows).tolist(), hi.tolist()))


def split_forward(case, rows, wrong=None):
    """The forward chain over ranks holding `rows` rows each (in order): what full_forward returns, y concatenated in rank order."""
    rows = np.asarray(rows, dtype=np.int64)
    assert int(rows.sum()) == case["x"].shape[0]
    cut = bounds(rows)
    partials = [stats(case["x"][lo:hi]) for lo, hi in cut]
    mean, invstd, rm, rv = combine(partials, rows, case["eps"], case["momentum"], case["running_mean"], case["running_var"], wrong)
    y = np.concatenate([apply(case["x"][lo:hi], case["residual"][lo:hi], case["gamma"], case["beta"], mean, invstd, case["flags"]) for lo, hi in cut])
    return dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv)


def split_backward(case, fwd, rows, wrong=None):
    """The backward chain: dx / dres concatenated in rank order; dgamma / dbeta the SUM of the ranks' local sums (what the gradient
    all-reduce makes of them, up to its 1 / world, which the loss's own 1 / rows undoes)."""
    rows = np.asarray(rows, dtype=np.int64)
    cut = bounds(rows)
    total, flags = int(rows.sum()), case["flags"]
    sums = np.stack([backward_reduce(case["dy"][lo:hi], case["x"][lo:hi], fwd["y"][lo:hi], fwd["mean"], fwd["invstd"], flags, wrong) for lo, hi in cut])
    parts = [backward_apply(case["dy"][lo:hi], case["x"][lo:hi], fwd["y"][lo:hi], case["gamma"], fwd["mean"], fwd["invstd"], sums, total, flags, wrong)
             for lo, hi in cut]
    dres = np.concatenate([p[1] for p in parts]) if flags & ADD else None
    return dict(dx=np.concatenate([p[0] for p in parts]), dres=dres, dgamma=sums[:, 1].sum(axis=0), dbeta=sums[:, 0].sum(axis=0))


def max_rel(a, b):
    """max |a - b| / max(1, max |b|): the error of a against b, relative to b's scale (never below 1)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    d = np.abs(a - b)
    return float("inf") if not np.isfinite(d).all() else float(d.max() / max(1.0, float(np.abs(b).max())))


def chain_errors(case, rows, wrong=None):
    """{name: max_rel} of the split chain over `rows` against full-batch BatchNorm, forward and backward."""
    ref = full_forward(case)
    ref_b = full_backward(case, ref)
    got = split_forward(case, rows, wrong)
    got_b = split_backward(case, got, rows, wrong)
    out = {k: max_rel(got[k], ref[k]) for k in ("y", "mean", "invstd", "running_mean", "running_var")}
    out.update({k: max_rel(got_b[k], ref_b[k]) for k in ("dx", "dgamma", "dbeta")})
    if case["flags"] & ADD:
        out["dres"] = max_rel(got_b["dres"], ref_b["dres"])
    return out
