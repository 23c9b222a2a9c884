"""SPEC M21 stated in numpy, written from the specification and not from the kernels: the nearest-code search, the
centroid update and k-means in float64, the update's chunk order a second time for the bit comparison, the per-row margin that
says where float32 may legitimately choose another code, and float32 restatements of the score and of the error.

(a)  n_k = 1/2 sum_d c_kd^2;  s(i,k) = n_k - sum_d x_id c_kd;  idx_i = the smallest k of minimal s;  err_i = sum_d (x_id - c_kd)^2.
     In float32 the score is the chain s = n_k; s = fmaf(-x_id, c_kd, s) over ascending d: D + 1 roundings (n_k's and one per
     step), each relative 2^-24 of a partial sum that is at most sum_d |x_id c_kd| + n_k in magnitude, so
         |s32 - s64| <= B(i,k) = (D + 2) 2^-24 (sum_d |x_id c_kd| + n_k)
     and a row is FLAGGED when its float64 gap between the best and the second-best code is under 2 max_k B(i,k): only there may
     float32 choose another code, and whatever it chooses scores within 2 max_k B of the minimum.
(b)  c_k = float32(sum w_i x_i / sum w_i) in double over the members of k; update_chunked() takes the sums in ascending row order
     within chunks of UPDATE_CHUNK consecutive members and adds the chunk partials in chunk order — the bits the kernels owe.
(c)  kmeans(): assign, update, reseed empty codes (the e-th empty code in ascending k takes the row of the e-th largest
     w_i err_i, stable descending sort), `iters` times, then a final assignment."""
import numpy as np

UPDATE_CHUNK = 256               # = VQ_UPDATE_CHUNK (tests/test_vq_cpu.py compares it with the header and the package)
U = 2.0 ** -24


def scores(x, c):
    """float64 [P,K]"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return 0.5 * (c * c).sum(1)[None, :] - x @ c.T


def assign(x, c):
    """(idx [P] int64: the first minimum, err [P] float64, scores [P,K] float64)"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    s = scores(x, c)
    idx = np.argmin(s, axis=1)             # numpy returns the first occurrence of the minimum
    err = ((x - c[idx]) ** 2).sum(1)
    return idx, err, s


def assign_brute(x, c):
    """the same by two loops and the squared distance itself, for the truth's own test"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    idx = np.zeros(len(x), np.int64)
    for i in range(len(x)):
        best = np.inf
        for k in range(len(c)):
            d = ((x[i] - c[k]) ** 2).sum()
            if d < best:
                best, idx[i] = d, k
    return idx


def bound(x, c):
    """max_k B(i,k) [P] float64"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    D = x.shape[1]
    n = 0.5 * (c * c).sum(1)
    return ((D + 2) * U * (np.abs(x) @ np.abs(c).T + n[None, :])).max(1)


def margins(x, c):
    """(gap [P]: second-best minus best float64 score, inf with one code; flagged [P] bool; bound [P])"""
    s = scores(x, c)
    b = bound(x, c)
    if s.shape[1] == 1:
        gap = np.full(len(s), np.inf)
    else:
        two = np.partition(s, 1, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
    return gap, gap < 2.0 * b, b


def scores_float32(x, c):
    """the sequential float32 chain of (a), each step formed exactly in float64 and rounded once to float32 (a float32 product is
    exact in float64; the sum of it and a float32 is rounded twice, which differs from fmaf on rare ties only) [P,K] float32"""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    n = (0.5 * (c.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    s = np.broadcast_to(n[None, :], (len(x), len(c))).copy()
    for d in range(x.shape[1]):
        s = (s.astype(np.float64) - x[:, d:d + 1].astype(np.float64) * c[None, :, d].astype(np.float64)).astype(np.float32)
    return s


def err_float32(x, c, idx):
    """e = 0; t = x - c (float32); e = fmaf(t, t, e) over ascending d, restated as above [P] float32"""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    e = np.zeros(len(x), np.float32)
    rows = c[np.asarray(idx, np.int64)]
    for d in range(x.shape[1]):
        t = (x[:, d] - rows[:, d]).astype(np.float32)
        e = (e.astype(np.float64) + t.astype(np.float64) ** 2).astype(np.float32)
    return e


def update(x, idx, c, w=None):
    """(new codebook float32 [K,D], mass float64 [K], count int64 [K]) with plain float64 sums (np.add.at order)"""
    x64, idx = np.asarray(x, np.float64), np.asarray(idx, np.int64)
    K, D = np.asarray(c).shape
    w64 = np.ones(len(x64)) if w is None else np.asarray(w, np.float64)
    num, mass = np.zeros((K, D)), np.zeros(K)
    np.add.at(num, idx, w64[:, None] * x64)
    np.add.at(mass, idx, w64)
    new = np.asarray(c, np.float32).copy()
    live = mass > 0
    new[live] = (num[live] / mass[live, None]).astype(np.float32)
    return new, mass, np.bincount(idx, minlength=K)


def update_chunked(x, idx, c, w=None):
    """(b) in the stated order: per code, the members in ascending row order; chunks of UPDATE_CHUNK consecutive members summed
    sequentially from 0.0 in double; chunk partials added in chunk order from 0.0; one division, one rounding"""
    x32, idx = np.asarray(x, np.float32), np.asarray(idx, np.int64)
    K, D = np.asarray(c).shape
    w32 = np.ones(len(x32), np.float32) if w is None else np.asarray(w, np.float32)
    new, mass = np.asarray(c, np.float32).copy(), np.zeros(K)
    count = np.bincount(idx, minlength=K)
    order = np.argsort(idx, kind="stable")
    start = 0
    for k in range(K):
        rows = order[start:start + count[k]]
        start += count[k]
        num, m = np.zeros(D), 0.0
        for a in range(0, len(rows), UPDATE_CHUNK):
            pn, pm = np.zeros(D), 0.0
            for i in rows[a:a + UPDATE_CHUNK]:
                wi = np.float64(w32[i])
                pn = pn + wi * x32[i].astype(np.float64)
                pm = pm + wi
            num, m = num + pn, m + pm
        mass[k] = m
        if m > 0:
            new[k] = (num / m).astype(np.float32)
    return new, mass, count


def reseed(x, c, count, w, err):
    """the e-th code without members, in ascending k, takes the row of the e-th largest w_i err_i (ties: the lower row)"""
    c = np.asarray(c, np.float32).copy()
    empty = np.flatnonzero(np.asarray(count) == 0)
    if len(empty):
        score = np.asarray(err, np.float64) * (1.0 if w is None else np.asarray(w, np.float64))
        worst = np.argsort(-score, kind="stable")[:len(empty)]
        c[empty] = np.asarray(x, np.float32)[worst]
    return c


def kmeans(x, init, iters, w=None, chunked=False):
    """(codebook float32, idx, history [iters + 1] of the weighted distortion, smallest (gap - 2 bound) over all assignments)"""
    c = np.asarray(init, np.float32).copy()
    w64 = np.ones(len(x)) if w is None else np.asarray(w, np.float64)
    history, slack = [], np.inf
    for _ in range(iters):
        idx, err, _ = assign(x, c)
        gap, _, b = margins(x, c)
        slack = min(slack, float((gap - 2.0 * b).min()))
        history.append(float((w64 * err).sum()))
        new, _, count = (update_chunked if chunked else update)(x, idx, c, w)
        c = reseed(x, new, count, w, err)
    idx, err, _ = assign(x, c)
    gap, _, b = margins(x, c)
    slack = min(slack, float((gap - 2.0 * b).min()))
    history.append(float((w64 * err).sum()))
    return c, idx, history, slack
