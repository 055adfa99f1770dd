"""not-gpu: the survivor bound of the dense top-k form (csrc/score.hip: k_dense_select) on numpy data.

The form keeps, per row, the items whose approximate (bf16) score is >= T - 2 eps, where eps is k_prep_x's bound on
|approx - exact| and T is the k-th largest of 256 per-thread maxima (thread t of the selection workgroup holds items
1024 q + 4 t + e).  Claim: the exact top-k (float32 fma chain, order by score descending then id ascending) is a subset of the
survivors.  Checked here for random catalogs and for the catalogs that stress the bound: all items equal, hundreds of copies of the
item that ranks k-th, items masked by a bias of -inf, rows scaled by 64 and by 1/64 (which moves eps)."""
import numpy as np
import pytest


def bf16_round(a):
    """float32 -> the float32 value of its bf16 rounding (round to nearest even, finite inputs): pack8_bf16's arithmetic"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return (u & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(np.shape(a))


def chain(x, W, b):
    """the exact score of every item for one row: float32 fma chain over k ascending, seeded with the bias (a float32 product is
    exact in float64; the one float64 rounding in front of the float32 one moves a result by at most one ulp, rarely)"""
    acc = b.astype(np.float32).copy()
    with np.errstate(invalid="ignore"):
        for k in range(x.shape[0]):
            acc = (np.float64(x[k]) * W[:, k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def w_norms(W, b):
    """k_pack_w's three maxima (float32 arithmetic, each rounded up by 1.001)"""
    Wr = bf16_round(W)
    f = np.float32
    ss = (W * W).sum(1, dtype=f)
    ssr = (Wr * Wr).sum(1, dtype=f)
    dw = W - Wr
    ssd = (dw * dw).sum(1, dtype=f)
    return (f(np.sqrt(np.maximum(ss, ssr)).max() * f(1.001)), f(np.sqrt(ssd).max() * f(1.001)), f(np.abs(b).max()))


def row_eps(x, wn, d_pad):
    """k_prep_x's eps of one row"""
    f = np.float32
    xr = bf16_round(x)
    dx = x - xr
    nx = f(np.sqrt(max((x * x).sum(dtype=f), (xr * xr).sum(dtype=f))))
    ndx = f(np.sqrt((dx * dx).sum(dtype=f)))
    acc_factor = f((d_pad + 8) * 2.0 ** -22)
    with np.errstate(invalid="ignore", over="ignore"):
        return f(f(1.001) * (ndx * wn[0] + nx * wn[1]) + acc_factor * (f(1.001) * nx * wn[0] + wn[2]))


def order_key(score, ids):
    """sort key of (score descending, id ascending) as one lexsort-able pair"""
    return np.lexsort((ids, -score.astype(np.float64)))


def survivors(approx, eps, k):
    """k_dense_select's survivor set for one row of approximate scores"""
    n = approx.shape[0]
    thr = np.float32(-np.inf)
    if n >= 4 * k:
        ids = np.arange(n)
        thread = (ids % 1024) // 4
        best = []  # per thread: (score, -id) of its largest key
        for t in range(256):
            m = ids[thread == t]
            if m.size:
                o = order_key(approx[m], m)[0]
                best.append((approx[m][o], m[o]))
        assert len(best) >= k
        sc = np.array([s for s, _ in best], dtype=np.float32)
        ii = np.array([i for _, i in best])
        T = sc[order_key(sc, ii)[k - 1]]
        with np.errstate(invalid="ignore"):
            thr = np.float32(T - np.float32(2.0) * eps)
    with np.errstate(invalid="ignore"):
        return ~(approx < thr)


def check(W, b, X, k):
    n, d = W.shape
    d_pad = (d + 15) // 16 * 16
    wn = w_norms(W, b)
    Wr = bf16_round(W)
    worst = 0
    for x in X:
        xr = bf16_round(x)
        with np.errstate(invalid="ignore"):
            approx = (Wr.astype(np.float32) @ xr.astype(np.float32) + b).astype(np.float32)
        exact = chain(x, W, b)
        eps = row_eps(x, wn, d_pad)
        fin = np.isfinite(exact)
        if np.isfinite(eps):
            assert np.abs(approx[fin].astype(np.float64) - exact[fin].astype(np.float64)).max() <= eps  # the premise
        keep = survivors(approx, eps, k)
        top = order_key(exact, np.arange(n))[:min(k, n)]
        assert keep[top].all(), (n, d, k, int((~keep[top]).sum()))
        worst = max(worst, int(keep.sum()))
    return worst


@pytest.mark.parametrize("n,d,k", [(99, 32, 100), (100, 64, 100), (101, 128, 100), (1000, 64, 100), (3415, 128, 100),
                                   (4065, 32, 256), (4096, 128, 1), (3415, 256, 256)])
def test_random_catalogs(n, d, k):
    rng = np.random.default_rng(n * 1000 + d + k)
    W = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(n) * 0.05).astype(np.float32)
    X = rng.standard_normal((6, d)).astype(np.float32)
    kept = check(W, b, X, k)
    if n >= 4 * k and k == 100 and n == 3415:
        assert kept < 1024  # an ordinary catalog stays far from the exhaustive path


def test_all_items_equal():
    rng = np.random.default_rng(1)
    W = np.repeat((rng.standard_normal((1, 128)) * 0.1).astype(np.float32), 3415, axis=0)
    b = np.zeros(3415, dtype=np.float32)
    assert check(W, b, rng.standard_normal((4, 128)).astype(np.float32), 100) == 3415  # every score ties: everything survives


def test_copies_of_the_kth_item():
    rng = np.random.default_rng(2)
    n, d, k = 3415, 128, 100
    W = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(n) * 0.05).astype(np.float32)
    X = rng.standard_normal((4, d)).astype(np.float32)
    for x in X:
        e = chain(x, W, b)
        kth = order_key(e, np.arange(n))[k - 1]
        W2, b2 = W.copy(), b.copy()
        spots = rng.choice(np.setdiff1d(np.arange(n), [kth]), 300, replace=False)
        W2[spots], b2[spots] = W[kth], b[kth]
        check(W2, b2, x[None], k)


def test_masked_items():
    rng = np.random.default_rng(3)
    n, d, k = 1000, 64, 100
    W = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(n) * 0.05).astype(np.float32)
    b[rng.choice(n, 50, replace=False)] = -np.inf
    check(W, b, rng.standard_normal((4, d)).astype(np.float32), k)


@pytest.mark.parametrize("scale", [64.0, 1.0 / 64.0])
def test_scaled_rows(scale):
    rng = np.random.default_rng(4)
    n, d, k = 3415, 128, 100
    W = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(n) * 0.05).astype(np.float32)
    check(W, b, (rng.standard_normal((4, d)) * scale).astype(np.float32), k)
