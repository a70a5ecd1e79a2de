"""Yardsticks for the SSM entries (include/ggml_hip_ext.h, SSM; csrc/ssm.hip): the statement of ggml_hip_ssm_scan_ragged_dev in float64, a float32 model of
it, the bar both are compared under, four mutants of the statement and two of the kernel's form, and the conv's statement with an exact binary32 fma.  Everything is for ONE sequence:
the ragged batch, the slots and the fresh / continued rule are the tests' business.

THE STATEMENT (per token t, head h, row p, state n; g = h // (n_head // G)):
    d = dt + dt_bias;  delta = d <= 20 ? log1p(exp(d)) : d;  a_n = exp(delta * A_n);  h_n = h_n * a_n + (delta * x) * B_n;  y = sum_n h_n C_n + D x

THE BAR.  u = 2^-24 is the unit roundoff of binary32; expf and log1pf are taken as 1 ulp, which is at most 2u relative.  Inputs are exact binary32 values.
Hats are computed values; every bound is first order in u except where |h| + E is written, which keeps the computed magnitude.

  d.      One addition: d^ = d (1 + e), |e| <= u (no error without a bias; the bound keeps it).
  delta.  softplus' = sigmoid, so the error of d moves softplus by at most |d| u sigmoid(d).  sigmoid(d) <= softplus(d) for every d (log(1 + z) >= z / (1 + z))
          and d sigmoid(d) <= softplus(d) for d >= 0, so that is at most max(1, |d|) u RELATIVE to delta.  expf: 2u relative on z = e^d, which moves
          log(1 + z) by 2u z / (1 + z) = 2u sigmoid <= 2u delta.  log1pf itself: 2u.  Together
              delta^ = delta (1 + eta),   |eta| <= kd u,   kd = 4 + max(1, |d|)            (the branch d > 20 has eta = e: inside the bound)
  a.      delta^ * A is one multiplication: relative (kd + 1) u on the ARGUMENT, i.e. an absolute (kd + 1) u |delta A| on it, which is that much relative
          on e^arg; expf adds 2u:
              a^ = a (1 + alpha),   |alpha| <= ka u,   ka = 2 + (kd + 1) |delta A|
  input.  (delta^ * x) * B is two multiplications: relative (kd + 2) u on delta x B.
  state.  h_t^ = fma(h_{t-1}^, a^, input^) is ONE rounding of the exact h_{t-1}^ a^ + input^, so with E_t = |h_t^ - h_t| and 0 < a <= 1 (A <= 0; the
          recurrence does not amplify)
              F_t = E_{t-1} a + ka u (|h_{t-1}| + E_{t-1}) a + (kd + 2) u |delta x B| + TINY (1 + |h_{t-1}| + E_{t-1})
              E_t = F_t + u (|h_t| + F_t)
          -- the inherited error damped by a, the error of a against the COMPUTED previous state, the error of the input, and the fma's own rounding
          of the computed h_t.  TINY = 2^-125: a, the input and h_t may land in the subnormal range, where a result carries an absolute error of up to
          2^-126 if the implementation flushes it (2^-149 if not) instead of a relative one; a's is multiplied by the previous state.
  y.      A slice is one product and 15 fmas, the butterfly adds log2(LP) additions (LP the least power of two >= N / 16): no term passes through more
          than ky = 16 + log2(LP) roundings, so by the usual bound for a sum of products |s^ - sum h^ C| <= ky u sum |h^ C|; the fma with D is one more
          rounding of the final value:
              bar(y) = sum_n E_n |C_n| + (ky + 1) u (sum_n (|h_n| + E_n) |C_n| + |D x|) + TINY
  The kernels are held to 1 x bar(y) for every output and to 1 x E_T for every element of the final state.  The bar is never measured from a kernel.
  The float32 model below is held to the same bars (tests/test_ssm.py)."""
import numpy as np

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -125
MUTANTS = ("no_softplus", "swap_bc", "group_off_by_one", "drop_D")
# mistakes only a kernel form can make, which no mutant of the statement resembles: the butterfly one step short (lane 0 of a group of LP lanes never meets
# the slices j with j & (LP / 2); judged where LP >= 2), and every state taking the A of state 0 (the per-state index lost; judged where A is per state)
KERNEL_MUTANTS = ("short_butterfly", "a_of_state_0")


def lanes_per_row(N):
    """LP: the least power of two >= N / 16"""
    LP = 1
    while LP < N // 16:
        LP *= 2
    return LP


def fmaf(a, b, c):
    """the exact binary32 fma of float32 arrays: a * b is exact in binary64, the sum is rounded TO ODD in binary64 (TwoSum tells whether it was exact and on
    which side the rest lies), and rounding a 53-bit round-to-odd value to 24 bits is the correctly rounded result"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        other = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    even = (s.view(np.int64) & 1) == 0
    s = np.where(np.isfinite(s) & (e != 0) & even, other, s)
    return s.astype(F)


def _expf(v):
    return np.exp(v.astype(np.float64)).astype(F)


def _group_of(n_head, G, mutant):
    g = np.arange(n_head) // (n_head // G)
    return (g + 1) % G if mutant == "group_off_by_one" else g


def scan_f64(x, dt, A, B, C, D=None, dt_bias=None, h0=None, mutant=None, want_bar=False):
    """the statement in float64 for one sequence.  x [T, H, P], dt [T, H], A [H] or [H, N], B / C [T, G, N], D / dt_bias [H] or None, h0 [H, P, N] or None
    (zeros).  -> (y [T, H, P], h [H, P, N]) and with want_bar the bars (bar_y, bar_h) of the docstring above, all float64.  mutant: one of MUTANTS or of
    KERNEL_MUTANTS"""
    x, dt, A, B, C = (np.asarray(v, np.float64) for v in (x, dt, A, B, C))
    T, H, P = x.shape
    G, N = B.shape[1:]
    g = _group_of(H, G, mutant)
    if mutant == "swap_bc":
        B, C = C, B
    An = (A[:, None] if A.ndim == 1 else A)[:, None, :]              # [H, 1, N or 1]
    if mutant == "a_of_state_0":
        An = An[:, :, :1]
    h = np.zeros((H, P, N)) if h0 is None else np.asarray(h0, np.float64).copy()
    E = np.zeros((H, P, N))
    y = np.zeros((T, H, P))
    bar_y = np.zeros((T, H, P))
    LP = lanes_per_row(N)
    ky = 16 + int(np.log2(LP))
    met = np.ones(N)                                                 # the states whose slice reaches lane 0 of the group
    if mutant == "short_butterfly":
        met = ((np.arange(N) // 16 & (LP // 2)) == 0).astype(np.float64)
    for t in range(T):
        d = dt[t] + (0.0 if dt_bias is None else np.asarray(dt_bias, np.float64))
        delta = d if mutant == "no_softplus" else np.where(d <= 20.0, np.log1p(np.exp(np.minimum(d, 20.0))), d)
        dA = delta[:, None, None] * An
        a = np.exp(dA)
        inp = (delta[:, None] * x[t])[:, :, None] * B[t][g][:, None, :]
        if want_bar:
            kd = 4.0 + np.maximum(1.0, np.abs(d))[:, None, None]
            ka = 2.0 + (kd + 1.0) * np.abs(dA)
            Fe = E * a + ka * U * (np.abs(h) + E) * a + (kd + 2.0) * U * np.abs(inp) + TINY * (1.0 + np.abs(h) + E)
        h = h * a + inp
        Ct = C[t][g][:, None, :]
        y[t] = (h * Ct * met).sum(-1)
        Dx = 0.0
        if D is not None and mutant != "drop_D":
            Dx = np.asarray(D, np.float64)[:, None] * x[t]
            y[t] += Dx
        if want_bar:
            E = Fe + U * (np.abs(h) + Fe)
            bar_y[t] = (E * np.abs(Ct)).sum(-1) + (ky + 1) * U * (((np.abs(h) + E) * np.abs(Ct)).sum(-1) + np.abs(Dx)) + TINY
    return (y, h, bar_y, E) if want_bar else (y, h)


def scan_f32(x, dt, A, B, C, D=None, dt_bias=None, h0=None):
    """the float32 model of the statement for one sequence, every operation one binary32 rounding in the header's order (expf / log1pf modelled as the
    correctly rounded functions): the slices of 16, the butterfly.  Arguments as scan_f64's, float32.  -> (y, h) float32"""
    x, dt, A, B, C = (np.asarray(v, F) for v in (x, dt, A, B, C))
    T, H, P = x.shape
    G, N = B.shape[1:]
    L = N // 16
    LP = lanes_per_row(N)
    g = _group_of(H, G, None)
    An = (A[:, None] if A.ndim == 1 else A)[:, None, :]
    h = np.zeros((H, P, N), F) if h0 is None else np.asarray(h0, F).copy()
    y = np.zeros((T, H, P), F)
    j = np.arange(LP)
    for t in range(T):
        d = dt[t] if dt_bias is None else dt[t] + np.asarray(dt_bias, F)
        sp = np.log1p(_expf(np.minimum(d, F(20.0))).astype(np.float64)).astype(F)
        delta = np.where(d <= F(20.0), sp, d).astype(F)
        a = _expf(delta[:, None, None] * An)
        dx = delta[:, None] * x[t]                                   # [H, P]
        h = fmaf(h, a, dx[:, :, None] * B[t][g][:, None, :])
        Ct = np.broadcast_to(C[t][g][:, None, :], h.shape).reshape(H, P, L, 16)
        hs = h.reshape(H, P, L, 16)
        s = hs[..., 0] * Ct[..., 0]
        for i in range(1, 16):
            s = fmaf(hs[..., i], Ct[..., i], s)
        sl = np.zeros((H, P, LP), F)
        sl[..., :L] = s
        k = 1
        while k < LP:
            sl = sl + sl[..., j ^ k]
            k *= 2
        yt = sl[..., 0]
        if D is not None:
            yt = fmaf(np.asarray(D, F)[:, None], x[t], yt)
        y[t] = yt
    return y, h


def conv_f32(x, w, bias=None, win0=None):
    """the conv's statement for one sequence, bit for bit (act = 0): x [T, n_ch], w [n_ch, d_conv], bias [n_ch] or None, win0 [d_conv - 1, n_ch] or None (a
    fresh sequence: zeros).  -> (acc [T, n_ch] float32, the new window [d_conv - 1, n_ch])"""
    x, w = np.asarray(x, F), np.asarray(w, F)
    T, n_ch = x.shape
    K = w.shape[1]
    win = np.concatenate([np.zeros((K - 1, n_ch), F) if win0 is None else np.asarray(win0, F), x])
    acc = w[:, 0] * win[0:T]
    for k in range(1, K):
        acc = fmaf(w[:, k], win[k:k + T], acc)
    if bias is not None:
        acc = acc + np.asarray(bias, F)
    return acc.astype(F), win[T:].copy()


def silu64(acc):
    """the silu of the conv's binary32 bits in float64: act = 1 is held to 3 u relative of it"""
    v = np.asarray(acc, np.float64)
    return v / (1.0 + np.exp(-v))
