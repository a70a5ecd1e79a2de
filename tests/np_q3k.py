"""numpy restatement of the PUBLISHED upstream Q3_K format (ggml k_quants.c, 2023-06: block_q3_K, dequantize_row_q3_K,
quantize_row_q3_K_reference with make_q3_quants, ggml_vec_dot_q3_K_q8_K) -- what kquants.hip's Q3_K kernels follow.

TEST INFRASTRUCTURE and the only checker there is: the reference has no k-quants and nothing here was run
against upstream -- PARITY UNPINNED, like tests/np_kquants.py for the other three.  Every float operation below is a binary32
operation in upstream's order; nearest = round half to even (np.rint).

    block_q3_K = { u8 hmask[32]; u8 qs[64]; u8 scales[12]; half d }      110 bytes per 256 weights
    element e: n = e / 128, s = (e % 128) / 32, l = e % 32
        v = ((qs[32 n + l] >> 2 s) & 3) + 4 ((hmask[l] >> (4 n + s)) & 1) - 4          (-4..3)
    scale j (elements 16 j .. 16 j + 15): code = (scales[j] & 15 | scales[j - 8] >> 4) | ((scales[8 + j % 4] >> 2 (j / 4)) & 3) << 4,
        sc_j = code - 32
    y[e] = (d * sc_j) * v"""
import numpy as np

import np_kquants as KQ

Q3K_BYTES = 110
F = np.float32


def q3_values(blocks):
    """[nb, 110] -> the signed 3-bit values v [nb, 256] int32 in element order"""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, Q3K_BYTES)
    hm = blocks[:, 0:32].astype(np.int32)
    qs = blocks[:, 32:96].astype(np.int32).reshape(-1, 2, 32)               # [nb, n, l]
    out = np.empty((blocks.shape[0], 2, 4, 32), dtype=np.int32)              # [nb, n, s, l]
    for n in range(2):
        for s in range(4):
            out[:, n, s] = ((qs[:, n] >> (2 * s)) & 3) + 4 * ((hm >> (4 * n + s)) & 1) - 4
    return out.reshape(-1, 256)


def q3_scale_codes(scale_bytes):
    """[..., 12] uint8 -> the sixteen 6-bit codes [..., 16] int32 (sc_j = code - 32)"""
    b = np.asarray(scale_bytes).astype(np.int32)
    out = np.empty(b.shape[:-1] + (16,), dtype=np.int32)
    for j in range(16):
        lo = (b[..., j] & 15) if j < 8 else (b[..., j - 8] >> 4)
        out[..., j] = lo | (((b[..., 8 + j % 4] >> (2 * (j // 4))) & 3) << 4)
    return out


def pack_scale_codes(codes):
    """inverse of q3_scale_codes: codes [..., 16] in 0..63 -> [..., 12] uint8"""
    c = np.asarray(codes).astype(np.int32)
    out = np.zeros(c.shape[:-1] + (12,), dtype=np.int32)
    for j in range(16):
        if j < 8:
            out[..., j] |= c[..., j] & 15
        else:
            out[..., j - 8] |= (c[..., j] & 15) << 4
        out[..., 8 + j % 4] |= (c[..., j] >> 4) << (2 * (j // 4))
    return out.astype(np.uint8)


def q3_scales(blocks):
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, Q3K_BYTES)
    return q3_scale_codes(blocks[:, 96:108]) - 32


def q3_d(blocks):
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, Q3K_BYTES)
    return blocks[:, 108:110].copy().view(np.float16).astype(F).reshape(-1)


def dequantize_q3_K(blocks):
    """[nb, 110] -> [nb, 256] f32: y = (d * sc_j) * v, the product d * sc_j first"""
    v = q3_values(blocks).reshape(-1, 16, 16).astype(F)
    ds = (q3_d(blocks)[:, None] * q3_scales(blocks).astype(F)).astype(F)
    return (ds[:, :, None] * v).astype(F).reshape(-1, 256)


def pack_q3(L):
    """codes L [nb, 256] in 0..7 -> (hmask [nb, 32], qs [nb, 64]) uint8: hmask[e % 32] bit e / 32 = L[e] > 3,
    qs[32 n + l] = (L & 3)[128 n + l] | [.. + 32] << 2 | [.. + 64] << 4 | [.. + 96] << 6"""
    L = np.asarray(L).astype(np.int32).reshape(-1, 8, 32)                   # [nb, e / 32, e % 32]
    hm = np.zeros((L.shape[0], 32), dtype=np.int32)
    for g in range(8):
        hm |= (L[:, g] >> 2) << g
    low = (L & 3).reshape(-1, 2, 4, 32)                                     # [nb, n, s, l]
    qs = np.zeros((L.shape[0], 2, 32), dtype=np.int32)
    for s in range(4):
        qs |= low[:, :, s] << (2 * s)
    return hm.astype(np.uint8), qs.reshape(-1, 64).astype(np.uint8)


def pack_q3_K(L, codes, d16):
    """codes L [nb, 256] (0..7), scale codes [nb, 16] (0..63), d [nb] float16 -> [nb, 110] super-blocks"""
    nb = np.asarray(L).reshape(-1, 256).shape[0]
    out = np.zeros((nb, Q3K_BYTES), dtype=np.uint8)
    out[:, 0:32], out[:, 32:96] = pack_q3(L)
    out[:, 96:108] = pack_scale_codes(codes)
    out[:, 108:110] = np.asarray(d16, dtype=np.float16).reshape(-1, 1).view(np.uint8)
    return out


def transcode_to_q6_K(blocks):
    """the exact Q3_K -> Q6_K transcoder: q6 = v + 32, scales[j] = sc_j (int8), the same d -- the same weights and the same planes"""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, Q3K_BYTES)
    out = np.zeros((blocks.shape[0], KQ.Q6K_BYTES), dtype=np.uint8)
    out[:, 0:128], out[:, 128:192] = KQ.pack_q6(q3_values(blocks) + 32)
    out[:, 192:208] = q3_scales(blocks).astype(np.int8).view(np.uint8)
    out[:, 208:210] = blocks[:, 108:110]
    return out


def mul_mat_q3_K(wrows, x):
    """wrows [M, K/256*110] uint8, x [N, K] f32 -> [N, M]: ggml_vec_dot_q3_K_q8_K per element -- per super-block
    (d * dy) * sum_j sc_j <v_j, a_j>, the integer sums exact; evaluated in f64 (a checker for the path's tolerance, not a bit-level one)"""
    M = wrows.shape[0]
    N, K = x.shape
    nb = K // 256
    d8, q8, _ = KQ.quantize_q8_K(x.reshape(-1, 256))
    d8, q8 = d8.reshape(N, nb).astype(np.float64), q8.reshape(N, nb, 16, 16).astype(np.float64)
    w = np.ascontiguousarray(wrows, dtype=np.uint8).reshape(M * nb, Q3K_BYTES)
    dw = q3_d(w).astype(np.float64).reshape(M, nb)
    sc = q3_scales(w).astype(np.float64).reshape(M, nb, 16)
    v = q3_values(w).astype(np.float64).reshape(M, nb, 16, 16)
    dots = np.einsum("mbjl,nbjl->nmbj", v, q8)
    isum = (dots * sc[None]).sum(axis=3)
    return (dw[None] * d8[:, None, :] * isum).sum(axis=2).astype(np.float32)


def make_q3_quants(x, passes=5):
    """make_q3_quants(16, nmax = 4, x, L, do_rmse = true) per row of x [ns, 16] -> (scale [ns] f32, L [ns, 16] int64 in 0..7).
    An all-zero sub-block gives L = 0 and scale 0.  `passes` = 0 skips the refinement (for the tests only).  A pass that accepts no
    change leaves the state as it found it, so running every pass is the same as upstream's early exit."""
    x = np.ascontiguousarray(x, dtype=F).reshape(-1, 16)
    ns = x.shape[0]
    ax = np.abs(x)
    idx = np.argmax(ax, axis=1)                                              # the first element of largest magnitude
    mx = x[np.arange(ns), idx]
    nz = ax[np.arange(ns), idx] != 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iscale = np.where(nz, (F(-4) / mx).astype(F), F(0)).astype(F)
        L = np.clip(np.rint((iscale[:, None] * x).astype(F)), -4, 3).astype(np.int64)
        w = (x * x).astype(F)
        wx = (w * x).astype(F)
        sumlx = np.zeros(ns, dtype=F)
        suml2 = np.zeros(ns, dtype=F)
        for i in range(16):
            Lf = L[:, i].astype(F)
            sumlx = (sumlx + (wx[:, i] * Lf).astype(F)).astype(F)
            suml2 = (suml2 + ((w[:, i] * Lf).astype(F) * Lf).astype(F)).astype(F)
        for _ in range(passes):
            for i in range(16):
                Lf = L[:, i].astype(F)
                slx = (sumlx - (wx[:, i] * Lf).astype(F)).astype(F)
                pos = slx > 0
                sl2 = (suml2 - ((w[:, i] * Lf).astype(F) * Lf).astype(F)).astype(F)
                r = ((x[:, i] * sl2).astype(F) / np.where(pos, slx, F(1))).astype(F)
                nl = np.clip(np.rint(np.where(pos, r, F(0))), -4, 3).astype(np.int64)
                nlf = nl.astype(F)
                slx2 = (slx + (wx[:, i] * nlf).astype(F)).astype(F)
                sl22 = (sl2 + ((w[:, i] * nlf).astype(F) * nlf).astype(F)).astype(F)
                better = ((slx2 * slx2).astype(F) * suml2).astype(F) > ((sumlx * sumlx).astype(F) * sl22).astype(F)
                acc = pos & (nl != L[:, i]) & (sl22 > 0) & better
                L[:, i] = np.where(acc, nl, L[:, i])
                sumlx = np.where(acc, slx2, sumlx).astype(F)
                suml2 = np.where(acc, sl22, suml2).astype(F)
        scale = np.where(nz, (sumlx / np.where(nz, suml2, F(1))).astype(F), F(0)).astype(F)
    return scale, np.where(nz[:, None], L + 4, 0)


def quantize_q3_K(x, passes=5):
    """quantize_row_q3_K_reference: x [nb, 256] f32 -> [nb, 110] super-blocks"""
    x = np.ascontiguousarray(x, dtype=F).reshape(-1, 256)
    nb = x.shape[0]
    xs = x.reshape(nb, 16, 16)
    scale, L = make_q3_quants(xs.reshape(-1, 16), passes)
    scale, L = scale.reshape(nb, 16), L.reshape(nb, 16, 16)
    j = np.argmax(np.abs(scale), axis=1)                                     # the first scale of largest magnitude
    max_scale = scale[np.arange(nb), j]
    zero = max_scale == 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        isc = np.where(zero, F(0), (F(-32) / np.where(zero, F(1), max_scale)).astype(F)).astype(F)
        d16 = np.where(zero, F(0), (F(1) / np.where(zero, F(1), isc)).astype(F)).astype(np.float16)
        codes = np.where(zero[:, None], 0, np.clip(np.rint((isc[:, None] * scale).astype(F)), -32, 31).astype(np.int64) + 32)
        dj = (d16.astype(F)[:, None] * (codes - 32).astype(F)).astype(F)   # the scale as the stored bytes give it
        live = dj != 0
        l2 = np.clip(np.rint((xs / np.where(live, dj, F(1))[:, :, None]).astype(F)), -4, 3).astype(np.int64) + 4
    L = np.where(live[:, :, None], l2, L)
    return pack_q3_K(L.reshape(nb, 256), codes, d16)


def weighted_error(x, blocks):
    """sum over elements of x^2 (y - x)^2 -- the error make_q3_quants' refinement lowers, measured after the whole quantizer"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 256)
    y = dequantize_q3_K(blocks).astype(np.float64)
    return float((x * x * (y - x) ** 2).sum())
