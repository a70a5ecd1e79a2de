"""Yardsticks for the CHUNKED selective scan (include/ggml_hip_ext.h, ggml_hip_ssm_scan_chunked_ragged_dev; csrc/ssm_chunk.hip): the bar its rows and final
state are held to against np_ssm.scan_f64 (the SEQUENTIAL statement in float64: the reference is not the code under test), a float32 model of the chunked
statement in the kernels' k order, and five mutants of the chunked form.  Everything is for ONE sequence whose chunks of Q tokens start at its first row.

THE CHUNKED STATEMENT (per head h, g its group; inside a chunk of L <= Q tokens, `last` = L - 1; H_in the state before the chunk):
    delta_t as np_ssm has it;  la_t = delta_t * A_h;  cs_t = cs_(t-1) + la_t (cs_(-1) = 0);  xd_s = delta_s * x_s
    S[p][n]     = sum_s (xd_s[p] * exp(cs_last - cs_s)) * B[s][n]               H_out = fma(H_in, exp(cs_last), S)
    G[t][s]     = sum_n C[t][n] B[s][n]                                         M[t][s] = exp(cs_t - cs_s) * G[t][s]  for s <= t, else 0
    y[t][p]     = sum_n (exp(cs_t) * C[t][n]) * H_in[p][n] + sum_(s <= t) M[t][s] * xd_s[p],  then fma(D, x, y)

THE BAR.  u = 2^-24; expf and log1pf are 1 ulp, at most 2u relative; inputs are exact binary32 values; hats are computed values.  First order in u, except
that an error d of an exponent's ARGUMENT is carried as expm1(d) on the exponential (d need not be small beside 1 where |cs| is large) and that a
magnitude next to an inherited error is written |v| + E.  The sequential bar (np_ssm) cannot serve: there the state has absorbed the cancellation over s
before anything is rounded against it, here every sum is rounded against the magnitudes of its terms.

  delta, la.  np_ssm: delta^ = delta (1 + eta), |eta| <= kd u, kd = 4 + max(1, |d|).  la^ = delta^ * A is one multiplication: |la^ - la| <= ela = (kd + 1) u |la|.
  cs.     cs_t^ = fl(cs_(t-1)^ + la_t^): every addition rounds against the RUNNING sum, |r_t| <= u |cs_t|.  So cs_t^ - cs_t = sum_(i <= t) (la_i^ - la_i + r_i):
              Ecs_t = sum_(i <= t) (ela_i + u |cs_i|)                            -- the rounding count is t + 1, each against |cs_i|, not against |la_i|
  decay.  cs_t^ - cs_s^ = (cs_t - cs_s) + sum_(s < i <= t) (la_i^ - la_i + r_i) EXACTLY (the errors up to s are common to both and cancel), and the
          subtraction rounds once more: the argument of exp(cs_t - cs_s) carries the ABSOLUTE error
              darg(t, s) = Ecs_t - Ecs_s + u |cs_t - cs_s|
          which becomes a RELATIVE error on the decay; expf adds 2u:
              rdec(t, s) = expm1(darg(t, s)) + 2u
          This is what the form costs: u |cs_i| is relative to how far the chunk has decayed since its START, however little it decays between s and t.
          exp(cs_t) alone (the H_in term, the state pass) is the same with s = -1: re(t) = expm1(Ecs_t) + 2u.
  xd.     delta^ * x: relative (kd + 1) u.
  S.      The A operand (xd_s^ * w_s^), w_s = exp(cs_last - cs_s), is one more multiplication: relative ra_s = (kd_s + 2) u + rdec(last, s).  The f32 MFMA is
          bit for bit a k-ordered fmaf chain from +0.0f: a term passes through at most L roundings, so with the usual bound for a sum of products
              ES[p][n] = sum_s |xd_s w_s B_s| (ra_s + L u) + TINY sum_s (1 + |B_s|)
          -- sum over s of MAGNITUDES; TINY = 2^-125 per operand and per step that may land in the subnormal range (np_ssm has the reason).
  state.  H_out^ = fma(H_in^, dec^, S^), dec = exp(cs_last), one rounding:
              F    = E_in dec + re(last) (|H_in| + E_in) dec + ES + TINY (1 + |H_in| + E_in)
              E_out = F + u (|H_out| + F)
          E_in = 0 for the first chunk (the slot holds exact binary32 values, or zeros); afterwards the E_out of the chunk before.
  G, M.   G is a chain of N products: EG = N u sum_n |C_t B_s| + N TINY.  M^ = fl(decay^ * G^):
              EM[t][s] = decay EG + |M| (rdec(t, s) + u) + TINY (1 + |G| + EG)
  y.      ONE chain of N + 16 ceil((t + 1) / 16) <= Ky = N + Q terms.  The H_in part: the A operand exp(cs_t)^ * C is relative re(t) + u; the inherited state
          error enters damped by exp(cs_t); the intra part carries EM and xd's error, summed over s as MAGNITUDES:
              Ey = sum_n e_t |C_n| ((re(t) + (Ky + 1) u) (|H_in| + E_in) + E_in) + sum_(s <= t) (EM |xd_s| + (|M| + EM) |xd_s| (kd_s + 1 + Ky) u)
                   + TINY (sum_n (1 + |H_in| + E_in) + sum_s (1 + |xd_s|))
              bar(y) = Ey + u (|y| + |D x| + Ey) + TINY                           -- the fma with D is one more rounding of the final value
  The kernels are held to 1 x bar(y) for every output and to 1 x E_out of the last chunk for every state element, and so is the float32 model below.  The bar
  is never measured from a kernel.

THE MUTANTS (mistakes this form invites; each exceeds the bar a hundredfold where it applies -- tests/test_ssm_chunk.py asserts both):
    mask_off_by_one      s < t instead of s <= t                                                  everywhere (y)
    end_decay_on_h_in    H_in reaches every row with the chunk's END decay exp(cs_last)            where H_in != 0 (y)
    no_decay_to_end      S without the weights exp(cs_last - cs_s)                                 the state everywhere; y from the second chunk
    tail_as_full         a partial tail treated as Q tokens, 3.0e38 in the rows behind it          partial tails (the state)
    quotient_decay       exp(cs_t) / exp(cs_s) from two binary32 exponentials                     where cs falls below expf's underflow (y)"""
import numpy as np

import np_ssm
from np_ssm import F, TINY, U, fmaf

MUTANTS = ("mask_off_by_one", "end_decay_on_h_in", "no_decay_to_end", "tail_as_full", "quotient_decay")
EXP_UNDERFLOW = -104.0                                              # below it the binary32 exponential is +0.0f


def _delta64(dt_c, dt_bias):
    d = dt_c + (0.0 if dt_bias is None else np.asarray(dt_bias, np.float64))
    return d, np.where(d <= 20.0, np.log1p(np.exp(np.minimum(d, 20.0))), d)


def chunk_f64(x, dt, A, B, C, D=None, dt_bias=None, h0=None, Q=64, mutant=None, want_bar=False):
    """the chunked statement in float64 for one sequence: x [T, H, P], dt [T, H], A [H], B / C [T, G, N], D / dt_bias [H] or None, h0 [H, P, N] or None.
    -> (y [T, H, P], h [H, P, N]); with want_bar (y, h, bar_y, bar_h, cs_min), the bars of the docstring and the least cs of any chunk.  mutant: one of MUTANTS"""
    x, dt, A, B, C = (np.asarray(v, np.float64) for v in (x, dt, A, B, C))
    T, H, P = x.shape
    G, N = B.shape[1:]
    g = np.arange(H) // (H // G)
    if mutant == "tail_as_full" and T % Q:
        pad = Q - T % Q
        x, dt, B, C = (np.concatenate([v, np.full((pad,) + v.shape[1:], 3.0e38)]) for v in (x, dt, B, C))
    h = np.zeros((H, P, N)) if h0 is None else np.asarray(h0, np.float64).copy()
    E = np.zeros((H, P, N))
    y = np.zeros((x.shape[0], H, P))
    bar_y = np.zeros((x.shape[0], H, P))
    cs_min = 0.0
    Ky = N + Q
    for c0 in range(0, x.shape[0], Q):
        xc, Bc, Cc = x[c0:c0 + Q], B[c0:c0 + Q][:, g], C[c0:c0 + Q][:, g]           # [L, H, P], [L, H, N]
        L = xc.shape[0]
        d, delta = _delta64(dt[c0:c0 + Q], dt_bias)                                # [L, H]
        with np.errstate(all="ignore"):
            la = delta * A
            cs = np.cumsum(la, 0)
            cs_min = min(cs_min, float(np.nanmin(cs)))
            xd = delta[:, :, None] * xc
            arg = cs[:, None] - cs[None]                                           # [t, s, H]
            causal = np.tril(np.ones((L, L), bool), -1 if mutant == "mask_off_by_one" else 0)[:, :, None]
            if mutant == "quotient_decay":
                e32 = np.exp(cs).astype(F)
                dec_ts = (e32[:, None] / e32[None]).astype(np.float64)
            else:
                dec_ts = np.exp(np.minimum(arg, 0.0))
            dec_ts = np.where(causal, dec_ts, 0.0)
            e_t = np.exp(cs)                                                       # [L, H]
            w = np.ones_like(cs) if mutant == "no_decay_to_end" else np.exp(cs[-1] - cs)
            Gm = np.einsum("thn,shn->tsh", Cc, Bc)
            M = np.where(causal, dec_ts * Gm, 0.0)
            e_h = np.broadcast_to(e_t[-1], e_t.shape) if mutant == "end_decay_on_h_in" else e_t
            CH = np.einsum("thn,hpn->thp", Cc, h)
            yc = e_h[:, :, None] * CH + np.einsum("tsh,shp->thp", M, xd)
            Dx = 0.0 if D is None else np.asarray(D, np.float64)[:, None] * xc
            S = np.einsum("shp,shn->hpn", xd * w[:, :, None], Bc)
            h_out = h * e_t[-1][:, None, None] + S
        if want_bar:
            kd = 4.0 + np.maximum(1.0, np.abs(d))                                  # [L, H]
            Ecs = np.cumsum((kd + 1.0) * U * np.abs(la) + U * np.abs(cs), 0)
            darg = Ecs[:, None] - Ecs[None] + U * np.abs(arg)                      # [t, s, H]
            rdec = np.expm1(np.where(causal, darg, 0.0)) + 2.0 * U
            re = np.expm1(Ecs) + 2.0 * U                                           # [L, H]
            # S and the state
            ra = (kd + 2.0) * U + rdec[-1]                                         # [s, H]
            ES = np.einsum("shp,shn->hpn", np.abs(xd * w[:, :, None]) * (ra + L * U)[:, :, None], np.abs(Bc)) + TINY * (L + np.abs(Bc).sum(0))[:, None, :]
            dec = e_t[-1][:, None, None]
            Fh = E * dec + re[-1][:, None, None] * (np.abs(h) + E) * dec + ES + TINY * (1.0 + np.abs(h) + E)
            E_out = Fh + U * (np.abs(h_out) + Fh)
            # y
            absCB = np.einsum("thn,shn->tsh", np.abs(Cc), np.abs(Bc))
            EG = N * U * absCB + N * TINY
            EM = np.where(causal, dec_ts * EG + np.abs(M) * (rdec + U) + TINY * (1.0 + np.abs(Gm) + EG), 0.0)
            hin = np.abs(h) + E
            t1 = e_t[:, :, None] * (np.einsum("thn,hpn->thp", np.abs(Cc), hin) * (re + (Ky + 1.0) * U)[:, :, None] + np.einsum("thn,hpn->thp", np.abs(Cc), E))
            axd = np.abs(xd)
            t2 = np.einsum("tsh,shp->thp", EM, axd) + np.einsum("tsh,shp->thp", np.abs(M) + EM, axd * ((kd + 1.0 + Ky) * U)[:, :, None])
            tiny = TINY * ((1.0 + hin).sum(-1)[None] + (1.0 + axd).sum(0)[None])
            Ey = t1 + t2 + tiny
            bar_y[c0:c0 + L] = Ey + U * (np.abs(yc + Dx) + np.abs(Dx) + Ey) + TINY
            E = E_out
        y[c0:c0 + L] = yc + Dx
        h = h_out
    y, bar_y = y[:T], bar_y[:T]
    return (y, h, bar_y, E, cs_min) if want_bar else (y, h)


def _expf(v):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(v, np.float64)).astype(F)


def n_order(N):
    """the order in which the kernels' MFMA chains visit n: 16 kb + 4 kq + c with kb, then c, then kq ascending"""
    return [16 * kb + 4 * kq + c for kb in range(N // 16) for c in range(4) for kq in range(4)]


def chunk_f32(x, dt, A, B, C, D=None, dt_bias=None, h0=None, Q=64):
    """the float32 model of the chunked statement for one sequence: every operation one binary32 rounding in the header's order (expf / log1pf modelled as
    the correctly rounded functions), the products as fmaf chains from +0.0f in the kernels' k order.  Arguments as chunk_f64's, float32.  -> (y, h) float32"""
    x, dt, A, B, C = (np.asarray(v, F) for v in (x, dt, A, B, C))
    T, H, P = x.shape
    G, N = B.shape[1:]
    g = np.arange(H) // (H // G)
    order = n_order(N)
    h = np.zeros((H, P, N), F) if h0 is None else np.asarray(h0, F).copy()
    y = np.zeros((T, H, P), F)
    for c0 in range(0, T, Q):
        xc, Bc, Cc = x[c0:c0 + Q], B[c0:c0 + Q][:, g], C[c0:c0 + Q][:, g]
        L = xc.shape[0]
        d = dt[c0:c0 + Q] if dt_bias is None else dt[c0:c0 + Q] + np.asarray(dt_bias, F)
        sp = np.log1p(_expf(np.minimum(d, F(20.0))).astype(np.float64)).astype(F)
        delta = np.where(d <= F(20.0), sp, d).astype(F)
        la = delta * A
        cs = np.zeros((L, H), F)
        run = np.zeros(H, F)
        for t in range(L):
            run = run + la[t]
            cs[t] = run
        w = _expf(cs[-1] - cs)                                                     # (one rounding of the difference, then expf)
        xd = delta[:, :, None] * xc
        xdw = xd * w[:, :, None]
        S = np.zeros((H, P, N), F)
        for s in range(L):
            S = fmaf(xdw[s][:, :, None], Bc[s][:, None, :], S)
        Gm = np.zeros((L, L, H), F)
        for n in order:
            Gm = fmaf(Cc[:, None, :, n], Bc[None, :, :, n], Gm)
        with np.errstate(over="ignore", invalid="ignore"):                        # (above the diagonal the difference is positive: masked, never used)
            M = np.where(np.tril(np.ones((L, L), bool))[:, :, None], _expf(cs[:, None] - cs[None]) * Gm, F(0.0)).astype(F)
        ec = _expf(cs)[:, :, None] * Cc                                            # [L, H, N]
        acc = np.zeros((L, H, P), F)
        for n in order:
            acc = fmaf(ec[:, :, n][:, :, None], h[None, :, :, n], acc)
        for s in range(L):
            acc = fmaf(M[:, s][:, :, None], xd[s][None], acc)
        if D is not None:
            acc = fmaf(np.asarray(D, F)[None, :, None], xc, acc)
        y[c0:c0 + L] = acc
        h = fmaf(h, _expf(cs[-1])[:, None, None], S)
    return y, h
