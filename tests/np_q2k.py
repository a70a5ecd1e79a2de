"""numpy restatement of the PUBLISHED upstream Q2_K format (ggml k_quants.c, 2023-06: block_q2_K, dequantize_row_q2_K,
quantize_row_q2_K_reference with make_qkx1_quants, ggml_vec_dot_q2_K_q8_K) -- what kquants.hip's Q2_K kernels follow -- and of the min
pass the library runs behind the block term's product.

TEST INFRASTRUCTURE and the only checker there is: the reference has no k-quants and nothing here was run
against upstream -- PARITY UNPINNED, like tests/np_kquants.py and tests/np_q3k.py.  Every float operation below is a binary32
operation in upstream's order; nearest = round half to even (np.rint).

    block_q2_K = { u8 scales[16]; u8 qs[64]; half d; half dmin }      84 bytes per 256 weights
    element e: n = e / 128, s = (e % 128) / 32, l = e % 32:  q = (qs[32 n + l] >> 2 s) & 3            (0..3)
    sub-block j = e / 16:  sc_j = scales[j] & 15,  m_j = scales[j] >> 4
    y[e] = (d * sc_j) * q - dmin * m_j"""
import numpy as np

import np_kquants as KQ

Q2K_BYTES = 84
F = np.float32


def q2_values(blocks):
    """[nb, 84] -> the 2-bit values q [nb, 256] int32 in element order"""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, Q2K_BYTES)
    qs = blocks[:, 16:80].astype(np.int32).reshape(-1, 2, 32)               # [nb, n, l]
    out = np.empty((blocks.shape[0], 2, 4, 32), dtype=np.int32)              # [nb, n, s, l]
    for s in range(4):
        out[:, :, s] = (qs >> (2 * s)) & 3
    return out.reshape(-1, 256)


def q2_scales(blocks):
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, Q2K_BYTES)
    return (blocks[:, 0:16] & 15).astype(np.int32)


def q2_mins(blocks):
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, Q2K_BYTES)
    return (blocks[:, 0:16] >> 4).astype(np.int32)


def q2_d(blocks):
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, Q2K_BYTES)
    return blocks[:, 80:82].copy().view(np.float16).astype(F).reshape(-1)


def q2_dmin(blocks):
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, Q2K_BYTES)
    return blocks[:, 82:84].copy().view(np.float16).astype(F).reshape(-1)


def dequantize_q2_K(blocks):
    """[nb, 84] -> [nb, 256] f32: dl = d * sc, ml = dmin * m, y = dl * q - ml (a multiply, then a subtract)"""
    q = q2_values(blocks).reshape(-1, 16, 16).astype(F)
    dl = (q2_d(blocks)[:, None] * q2_scales(blocks).astype(F)).astype(F)
    ml = (q2_dmin(blocks)[:, None] * q2_mins(blocks).astype(F)).astype(F)
    return ((dl[:, :, None] * q).astype(F) - ml[:, :, None]).astype(F).reshape(-1, 256)


def pack_q2(L):
    """codes L [nb, 256] in 0..3 -> qs [nb, 64] uint8: qs[32 n + l] = L[128 n + l] | L[.. + 32] << 2 | L[.. + 64] << 4 | L[.. + 96] << 6"""
    L = np.asarray(L).astype(np.int32).reshape(-1, 2, 4, 32)                # [nb, n, s, l]
    qs = np.zeros((L.shape[0], 2, 32), dtype=np.int32)
    for s in range(4):
        qs |= (L[:, :, s] & 3) << (2 * s)
    return qs.reshape(-1, 64).astype(np.uint8)


def pack_q2_K(L, sc, m, d16, dmin16):
    """codes L [nb, 256] (0..3), scales / mins [nb, 16] (0..15), d / dmin [nb] float16 -> [nb, 84] super-blocks"""
    nb = np.asarray(L).reshape(-1, 256).shape[0]
    out = np.zeros((nb, Q2K_BYTES), dtype=np.uint8)
    out[:, 0:16] = (np.asarray(sc).astype(np.int32) | (np.asarray(m).astype(np.int32) << 4)).astype(np.uint8)
    out[:, 16:80] = pack_q2(L)
    out[:, 80:82] = np.asarray(d16, dtype=np.float16).reshape(-1, 1).view(np.uint8)
    out[:, 82:84] = np.asarray(dmin16, dtype=np.float16).reshape(-1, 1).view(np.uint8)
    return out


def transcode_to_q6_K(blocks):
    """the block term as a Q6_K super-block: q6 = q + 32, scales[j] = sc_j, the same d (the min term is dropped)"""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, Q2K_BYTES)
    out = np.zeros((blocks.shape[0], KQ.Q6K_BYTES), dtype=np.uint8)
    out[:, 0:128], out[:, 128:192] = KQ.pack_q6(q2_values(blocks) + 32)
    out[:, 192:208] = q2_scales(blocks).astype(np.int8).view(np.uint8)
    out[:, 208:210] = blocks[:, 80:82]
    return out


def min_term(wrows, x):
    """T [N, M] f32 the min pass subtracts, in its own order: per (n, i) acc = +0; for sb ascending: S = sum_j m_j * bsum_j (exact integer),
    c = fl(dy * dmin), acc = fl(acc + fl(c * S)).  dy and bsum are quantize_q8_K's d and bsums."""
    M = wrows.shape[0]
    N, K = x.shape
    nb = K // 256
    d8, _, bsums = KQ.quantize_q8_K(np.ascontiguousarray(x, dtype=F).reshape(-1, 256))
    d8, bsums = d8.reshape(N, nb), bsums.reshape(N, nb, 16).astype(np.int64)
    w = np.ascontiguousarray(wrows, dtype=np.uint8).reshape(M * nb, Q2K_BYTES)
    dmin = q2_dmin(w).reshape(M, nb)
    m = q2_mins(w).reshape(M, nb, 16).astype(np.int64)
    acc = np.zeros((N, M), dtype=F)
    for sb in range(nb):
        S = (bsums[:, sb, :] @ m[:, sb, :].T).astype(F)                     # |S| < 2^19: exact
        c = (d8[:, sb][:, None] * dmin[:, sb][None, :]).astype(F)
        acc = (acc + (c * S).astype(F)).astype(F)
    return acc


def mul_mat_q2_K(wrows, x):
    """wrows [M, K/256*84] uint8, x [N, K] f32 -> [N, M]: ggml_vec_dot_q2_K_q8_K per element -- per super-block
    (d * dy) * sum_j sc_j <q_j, a_j> - (dmin * dy) * sum_j m_j bsum_j, evaluated in f64 (a checker for the path's tolerance, not a bit-level one)"""
    M = wrows.shape[0]
    N, K = x.shape
    nb = K // 256
    d8, q8, bsums = KQ.quantize_q8_K(np.ascontiguousarray(x, dtype=F).reshape(-1, 256))
    d8 = d8.reshape(N, nb).astype(np.float64)
    q8, bsums = q8.reshape(N, nb, 16, 16).astype(np.float64), bsums.reshape(N, nb, 16).astype(np.float64)
    w = np.ascontiguousarray(wrows, dtype=np.uint8).reshape(M * nb, Q2K_BYTES)
    dw, dmw = q2_d(w).astype(np.float64).reshape(M, nb), q2_dmin(w).astype(np.float64).reshape(M, nb)
    sc, m = q2_scales(w).astype(np.float64).reshape(M, nb, 16), q2_mins(w).astype(np.float64).reshape(M, nb, 16)
    q = q2_values(w).astype(np.float64).reshape(M, nb, 16, 16)
    isum = (np.einsum("mbjl,nbjl->nmbj", q, q8) * sc[None]).sum(axis=3)
    msum = np.einsum("mbj,nbj->nmb", m, bsums)
    return (d8[:, None, :] * (dw[None] * isum - dmw[None] * msum)).sum(axis=2).astype(np.float32)


def make_qkx1_quants(x, nmax, ntry=5):
    """make_qkx1_quants(n, nmax, x, L, &the_min, ntry) for rows x [ns, n] of any length n (np_kquants.make_qkx1_quants is the n = 32 case)
    -> (scale [ns], the_min [ns], L [ns, n] int64)"""
    x = np.ascontiguousarray(x, dtype=F)
    ns, n = x.shape
    mn = x.min(axis=1).astype(F)
    mx = x.max(axis=1).astype(F)
    flat = mx == mn
    mn = np.where(mn > 0, F(0), mn).astype(F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iscale = (F(nmax) / (mx - mn).astype(F)).astype(F)
        scale = (F(1) / iscale).astype(F)
        L = np.full((ns, n), -1, dtype=np.int64)
        live = ~flat
        for _ in range(ntry):
            if not live.any():
                break
            sumlx = np.zeros(ns, dtype=F)
            suml2 = np.zeros(ns, dtype=np.int64)
            changed = np.zeros(ns, dtype=bool)
            Lnew = L.copy()
            for i in range(n):
                t = (x[:, i] - mn).astype(F)
                l = np.clip(np.rint((iscale * t).astype(F)), 0, nmax).astype(np.int64)
                changed |= l != L[:, i]
                Lnew[:, i] = l
                sumlx = (sumlx + (t * l.astype(F)).astype(F)).astype(F)
                suml2 += l * l
            sc_new = (sumlx / suml2.astype(F)).astype(F)
            s = np.zeros(ns, dtype=F)
            for i in range(n):
                s = (s + (x[:, i] - (sc_new * Lnew[:, i].astype(F)).astype(F)).astype(F)).astype(F)
            mn_new = (s / F(n)).astype(F)
            mn_new = np.where(mn_new > 0, F(0), mn_new).astype(F)
            L = np.where(live[:, None], Lnew, L)
            scale = np.where(live, sc_new, scale).astype(F)
            mn = np.where(live, mn_new, mn).astype(F)
            iscale = np.where(live, (F(1) / scale).astype(F), iscale).astype(F)
            live = live & changed
    L = np.where(flat[:, None], 0, L)
    return np.where(flat, F(0), scale).astype(F), np.where(flat, F(0), -mn).astype(F), L


def quantize_q2_K(x):
    """quantize_row_q2_K_reference: x [nb, 256] f32 -> [nb, 84] super-blocks"""
    x = np.ascontiguousarray(x, dtype=F).reshape(-1, 256)
    nb = x.shape[0]
    xs = x.reshape(nb, 16, 16)
    scale, mins, L = make_qkx1_quants(xs.reshape(-1, 16), 3)
    scale, mins, L = scale.reshape(nb, 16), mins.reshape(nb, 16), L.reshape(nb, 16, 16)
    max_scale = np.maximum(scale.max(axis=1), F(0)).astype(F)                # (upstream: `if (scale > max_scale)` from 0)
    max_min = np.maximum(mins.max(axis=1), F(0)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ps, pm = max_scale > 0, max_min > 0
        inv_s = np.where(ps, (F(15) / np.where(ps, max_scale, F(1))).astype(F), F(0)).astype(F)
        inv_m = np.where(pm, (F(15) / np.where(pm, max_min, F(1))).astype(F), F(0)).astype(F)
        ls = np.where(ps[:, None], np.clip(np.rint((inv_s[:, None] * scale).astype(F)), 0, 15), 0).astype(np.int64)
        lm = np.where(pm[:, None], np.clip(np.rint((inv_m[:, None] * mins).astype(F)), 0, 15), 0).astype(np.int64)
        d16 = np.where(ps, (max_scale / F(15)).astype(F), F(0)).astype(np.float16)
        dmin16 = np.where(pm, (max_min / F(15)).astype(F), F(0)).astype(np.float16)
        dd = (d16.astype(F)[:, None] * ls.astype(F)).astype(F)
        dm = (dmin16.astype(F)[:, None] * lm.astype(F)).astype(F)
        live = dd != 0
        l2 = np.clip(np.rint(((xs + dm[:, :, None]).astype(F) / np.where(live, dd, F(1))[:, :, None]).astype(F)), 0, 3)
    L = np.where(live[:, :, None], np.nan_to_num(l2).astype(np.int64), L)
    return pack_q2_K(L.reshape(nb, 256), ls, lm, d16, dmin16)
