"""The sampler of include/ggml_hip_ext.h (ggml_hip_argmax_rows_dev, ggml_hip_sample_topk_dev) restated in numpy: the yardsticks of
tests/test_decode_ends.py.

  topk_ids      exact: a stable sort by (NaN last, larger logit first, smaller index first); -0.0 == +0.0 (test_moe_route.py's rule);
  probs64       the header's formulas in float64 on the same f32 logits and the same f32 inv_temp;
  probs32       a numpy float32 MODEL of the statement (one binary32 rounding per operation, numpy's f32 exp for expf);
  keep_pick     exact: n_keep and the pick from a row of f32 probabilities by the sequential f32 sums the header states.

THE BOUND of probs against probs64, per slot s, derived from the statement and the number format alone (u = 2^-24, one binary32 rounding;
z_s = (l_s - l_0) * inv_temp <= 0, e_s = exp(z_s), S = sum e_t >= e_0 = 1):
  - l_s - l_0 is rounded once: half an ulp, u relative, which moves z_s by |z_s| u;   the product by inv_temp rounds once more: |z_s| u;
    an absolute error a in z is a relative error a in exp(z):                                          2 |z_s| u
  - expf is within 1 ulp = 2 u relative, in the numerator:                                                      2 u
  - the same two sources in every term of S, weighted by the term's share of S:       sum_t e_t (2 |z_t| + 2) u / S
  - k - 1 roundings in the sequential sum (every partial sum is <= S):                                    (k - 1) u
  - one rounding from the division:                                                                             u
  bound_s = (2 |z_s| + 2 + sum_t e_t (2 |z_t| + 2) / S + k) * u, first order; the second-order terms are below 2^-40 for |z| <= 60.
statistic() is max over slots of |p - p64| / (p64 * bound_s): the bar is 1.  Logits are drawn so that |z| <= Z_MAX = 60: no e_s is then
subnormal (exp(-60) = 8.8e-27) and the relative bound means something for every slot.
MODEL_WORST records what probs32 measures over test_decode_ends.py's cases on the CPU (test_the_model_constant_is_what_the_model_measures)."""
import numpy as np

U = 2.0 ** -24
Z_MAX = 60.0
MODEL_WORST = 0.44         # the worst statistic() of probs32 over the cases of test_decode_ends.py (0.4332, among 4096 rows at k = 2); the bar is 1.0


def topk_ids(logits, k):
    """[n_rows, k] int32: rank order under (a NaN after every number, larger logit first, smaller index first)"""
    l = np.asarray(logits, np.float32)
    isn = np.isnan(l)
    idx = np.broadcast_to(np.arange(l.shape[1]), l.shape)
    with np.errstate(invalid="ignore"):
        order = np.lexsort((idx, -np.where(isn, np.float32(0), l), isn), axis=1)       # (the last key is the primary one; -0.0 == 0.0)
    return order[:, :k].astype(np.int32)


def _z64(logits, ids, inv_temp):
    l = np.asarray(logits, np.float32).astype(np.float64)
    sel = np.take_along_axis(l, ids.astype(np.int64), axis=1)
    return (sel - sel[:, :1]) * float(np.float32(inv_temp))


def probs64(logits, ids, inv_temp):
    """[n_rows, k] float64"""
    e = np.exp(_z64(logits, ids, inv_temp))
    return e / e.sum(axis=1, keepdims=True)


def bound(logits, ids, inv_temp):
    """[n_rows, k] float64: the derived relative bound per slot (the docstring's bound_s)"""
    z = np.abs(_z64(logits, ids, inv_temp))
    e = np.exp(-z)
    share = (e * (2.0 * z + 2.0)).sum(axis=1, keepdims=True) / e.sum(axis=1, keepdims=True)
    return (2.0 * z + 2.0 + share + ids.shape[1]) * U


def statistic(probs, logits, ids, inv_temp):
    want = probs64(logits, ids, inv_temp)
    return float((np.abs(np.asarray(probs, np.float64) - want) / (want * bound(logits, ids, inv_temp))).max())


def spread(logits, ids, inv_temp):
    """the largest |z| of the selected slots: the generator must keep it <= Z_MAX"""
    return float(np.abs(_z64(logits, ids, inv_temp)).max())


def probs32(logits, ids, inv_temp):
    """the statement in float32: e_s = expf((l_s - l_0) * inv_temp), S sequential in rank order, p_s = e_s / S"""
    l = np.asarray(logits, np.float32)
    sel = np.take_along_axis(l, ids.astype(np.int64), axis=1)
    sel = np.where(sel == 0, np.float32(0), sel)                                       # (a zero is taken as +0.0)
    z = (sel - sel[:, :1]) * np.float32(inv_temp)
    e = np.exp(z)
    assert z.dtype == np.float32 and e.dtype == np.float32
    S = e[:, 0].copy()
    for s in range(1, e.shape[1]):
        S = S + e[:, s]
    p = e / S[:, None]
    assert p.dtype == np.float32
    return p


def keep_pick(p, top_p, u):
    """one row: p f32 [k] (the probabilities the entry wrote), top_p and u f32 -> (n_keep, the picked RANK), every sum a sequential f32 sum"""
    p = np.asarray(p, np.float32)
    top_p, u = np.float32(top_p), np.float32(u)
    k = p.shape[0]
    n_keep = k
    if not top_p >= np.float32(1):
        acc = p[0]
        for n in range(1, k + 1):
            if n > 1:
                acc = np.float32(acc + p[n - 1])
            if acc >= top_p:
                n_keep = n
                break
    C = p[0]
    for s in range(1, n_keep):
        C = np.float32(C + p[s])
    target = np.float32(u * C)
    run = p[0]
    for s in range(n_keep):
        if s > 0:
            run = np.float32(run + p[s])
        if run > target:
            return n_keep, s
    return n_keep, n_keep - 1
