"""numpy restatement of upstream's IQ4_NL and IQ4_XS formats (block_iq4_nl, block_iq4_xs, kvalues_iq4nl, dequantize_row_iq4_nl / _iq4_xs,
quantize_row_iq4_nl_impl without importance weights, ntry = 7) -- what ggmlsharp_amd/csrc/iq4.hip follows.

TEST INFRASTRUCTURE and the only checker there is: the reference has no IQ types and no upstream source is on hand, so this restates the
published algorithm as include/ggml_hip_ext.h states it -- PARITY UNPINNED, like tests/np_kquants.py.  Every float operation below is ONE
binary32 operation in the order written (vectorised over blocks, sequential over j inside a block); nearest = round half to even (np.rint).

    kv = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113}
    block_iq4_nl = { half d; u8 qs[16] }                                   18 bytes per 32 weights
        element j < 16: qs[j] & 15, element j + 16: qs[j] >> 4 (indices into kv);  y = d * kv[idx]
    block_iq4_xs = { half d; u16 scales_h; u8 scales_l[4]; u8 qs[128] }    136 bytes per 256 weights
        ls_ib = ((scales_l[ib / 2] >> 4 (ib % 2)) & 15) | (((scales_h >> 2 ib) & 3) << 4); qs[16 ib .. 16 ib + 15] as IQ4_NL's
        y = (d * (ls - 32)) * kv[idx]"""
import numpy as np

import np_kquants as KQ
import np_restatement as R

F = np.float32
KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], dtype=np.int32)
KVF = KV.astype(F)
IQ4NL_BYTES, IQ4XS_BYTES = 18, 136


# ---------------------------------------------------------------- the formats
def nibbles(qs):
    """[..., 16] uint8 -> the 32 codebook indices [..., 32] (element j < 16: low nibble of qs[j], j + 16: its high nibble)"""
    q = np.asarray(qs).astype(np.int32)
    return np.concatenate([q & 15, q >> 4], axis=-1)


def pack_nibbles(idx):
    idx = np.asarray(idx).astype(np.int32)
    return (idx[..., :16] | (idx[..., 16:] << 4)).astype(np.uint8)


def _half(b, off):
    return b[:, off:off + 2].copy().view(np.float16).astype(F).reshape(-1)


def _nl(blocks):
    return np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, IQ4NL_BYTES)


def _xs(blocks):
    return np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, IQ4XS_BYTES)


def iq4nl_index(blocks):
    return nibbles(_nl(blocks)[:, 2:18])


def iq4nl_values(blocks):
    return KV[iq4nl_index(blocks)]


def iq4nl_d(blocks):
    return _half(_nl(blocks), 0)


def dequantize_iq4_nl(blocks):
    """[nb, 18] -> [nb, 32] f32: y = d * kv[idx]"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (iq4nl_d(blocks)[:, None] * KVF[iq4nl_index(blocks)]).astype(F)


def pack_iq4_nl(idx, d16):
    idx = np.asarray(idx).reshape(-1, 32)
    out = np.zeros((idx.shape[0], IQ4NL_BYTES), dtype=np.uint8)
    out[:, 0:2] = np.asarray(d16, dtype=np.float16).reshape(-1, 1).view(np.uint8)
    out[:, 2:18] = pack_nibbles(idx)
    return out


def xs_codes(blocks):
    """[nb, 136] -> the eight 6-bit scale codes ls [nb, 8] int32"""
    b = _xs(blocks).astype(np.int32)
    sh = b[:, 2] | (b[:, 3] << 8)
    out = np.empty((b.shape[0], 8), dtype=np.int32)
    for ib in range(8):
        out[:, ib] = ((b[:, 4 + ib // 2] >> (4 * (ib % 2))) & 15) | (((sh >> (2 * ib)) & 3) << 4)
    return out


def pack_xs_codes(codes):
    """codes [nb, 8] in 0..63 -> the four header bytes scales_h (little-endian), scales_l[4] as [nb, 6] uint8"""
    c = np.asarray(codes).astype(np.int32).reshape(-1, 8)
    sh = np.zeros(c.shape[0], dtype=np.int32)
    sl = np.zeros((c.shape[0], 4), dtype=np.int32)
    for ib in range(8):
        sh |= (c[:, ib] >> 4) << (2 * ib)
        sl[:, ib // 2] |= (c[:, ib] & 15) << (4 * (ib % 2))
    return np.concatenate([(sh & 0xFF)[:, None], (sh >> 8)[:, None], sl], axis=1).astype(np.uint8)


def iq4xs_index(blocks):
    return nibbles(_xs(blocks)[:, 8:].reshape(-1, 8, 16))              # [nb, 8, 32]


def iq4xs_values(blocks):
    return KV[iq4xs_index(blocks)]


def iq4xs_d(blocks):
    return _half(_xs(blocks), 0)


def iq4xs_scales(blocks):
    """the effective sub-block scales d * (ls - 32) [nb, 8] f32 (exact)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (iq4xs_d(blocks)[:, None] * (xs_codes(blocks) - 32).astype(F)).astype(F)


def dequantize_iq4_xs(blocks):
    """[nb, 136] -> [nb, 256] f32: y = (d * (ls - 32)) * kv[idx]"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (iq4xs_scales(blocks)[:, :, None] * KVF[iq4xs_index(blocks)]).astype(F).reshape(-1, 256)


def pack_iq4_xs(idx, codes, d16):
    """indices [nb, 8, 32] (0..15), scale codes [nb, 8] (0..63), d [nb] float16 -> [nb, 136] super-blocks"""
    idx = np.asarray(idx).reshape(-1, 8, 32)
    out = np.zeros((idx.shape[0], IQ4XS_BYTES), dtype=np.uint8)
    out[:, 0:2] = np.asarray(d16, dtype=np.float16).reshape(-1, 1).view(np.uint8)
    out[:, 2:8] = pack_xs_codes(codes)
    out[:, 8:] = pack_nibbles(idx).reshape(-1, 128)
    return out


# ---------------------------------------------------------------- the exact transcoders
def transcode_iq4nl_to_q8_0(blocks):
    """IQ4_NL -> this library's Q8_0 block {f32 d; i8 qs[32]}: f32 d = the half d (exact), qs[j] = kv[idx_j] -- the same weights"""
    b = _nl(blocks)
    out = np.zeros((b.shape[0], 36), dtype=np.uint8)
    out[:, 0:4] = iq4nl_d(b).astype(F).view(np.uint8).reshape(-1, 4)
    out[:, 4:] = iq4nl_values(b).astype(np.int8).view(np.uint8)
    return out


def transcode_iq4xs_to_q6_K(blocks):
    """IQ4_XS whose values lie in -32..31 (indices 6..10) -> Q6_K: q6 = v + 32, scales[2 i] = scales[2 i + 1] = ls_i - 32, the same d"""
    b = _xs(blocks)
    v = iq4xs_values(b).reshape(-1, 256)
    assert v.min() >= -32 and v.max() <= 31, "only IQ4_XS values in -32..31 have a Q6_K twin"
    out = np.zeros((b.shape[0], KQ.Q6K_BYTES), dtype=np.uint8)
    out[:, 0:128], out[:, 128:192] = KQ.pack_q6(v + 32)
    out[:, 192:208] = np.repeat(xs_codes(b) - 32, 2, axis=1).astype(np.int8).view(np.uint8)
    out[:, 208:210] = b[:, 0:2]
    return out


# ---------------------------------------------------------------- the products (checkers for the path's tolerance, evaluated in f64)
def mul_mat_iq4_nl(wrows, x):
    """wrows [M, K/32*18] uint8, x [N, K] f32 -> [N, M]: per block (d_w * d_a) * <kv[idx], a> against this library's Q8_0 activations"""
    M = wrows.shape[0]
    N, K = x.shape
    nb = K // 32
    d1, a = R._q8_0_parts(R.quantize_q8_0(x))
    d1, a = d1.reshape(N, nb).astype(np.float64), a.reshape(N, nb, 32).astype(np.float64)
    w = _nl(wrows)
    d0 = iq4nl_d(w).astype(np.float64).reshape(M, nb)
    v = iq4nl_values(w).astype(np.float64).reshape(M, nb, 32)
    dots = np.einsum("mbj,nbj->nmb", v, a)
    return (d0[None] * d1[:, None, :] * dots).sum(axis=2).astype(np.float32)


def mul_mat_iq4_xs(wrows, x):
    """wrows [M, K/256*136] uint8, x [N, K] f32 -> [N, M]: per super-block (d * dy) * sum_ib (ls_ib - 32) <kv[idx_ib], a_ib> against Q8_K"""
    M = wrows.shape[0]
    N, K = x.shape
    nb = K // 256
    d8, q8, _ = KQ.quantize_q8_K(x.reshape(-1, 256))
    d8, q8 = d8.reshape(N, nb).astype(np.float64), q8.reshape(N, nb, 8, 32).astype(np.float64)
    w = _xs(wrows)
    dw = iq4xs_d(w).astype(np.float64).reshape(M, nb)
    sc = (xs_codes(w) - 32).astype(np.float64).reshape(M, nb, 8)
    v = iq4xs_values(w).astype(np.float64).reshape(M, nb, 8, 32)
    dots = np.einsum("mbjl,nbjl->nmbj", v, q8)
    return (dw[None] * d8[:, None, :] * (dots * sc[None]).sum(axis=3)).sum(axis=2).astype(np.float32)


# ---------------------------------------------------------------- the quantizer
def best_index(x):
    """best_index_int8(16, kv, x), literally: x <= kv[0] -> 0; x >= kv[15] -> 15; binary search (ml = 0, mu = 15 while mu - ml > 1:
    mav = (ml + mu) / 2, x < kv[mav] ? mu = mav : ml = mav); then (x - kv[mu - 1] < kv[mu] - x) ? mu - 1 : mu"""
    x = np.asarray(x, dtype=F)
    ml = np.zeros(x.shape, dtype=np.int64)
    mu = np.full(x.shape, 15, dtype=np.int64)
    while True:
        live = (mu - ml) > 1
        if not live.any():
            break
        mav = (ml + mu) // 2
        less = x < KVF[mav]
        mu = np.where(live & less, mav, mu)
        ml = np.where(live & ~less, mav, ml)
    with np.errstate(invalid="ignore", over="ignore"):
        lower = (x - KVF[mu - 1]).astype(F) < (KVF[mu] - x).astype(F)
    idx = np.where(lower, mu - 1, mu)
    return np.where(x <= KVF[0], 0, np.where(x >= KVF[15], 15, idx))


def _sums(xb, w, idv):
    """sumqx, sumq2 of a block under the inverse scale idv: q = kv[best_index(idv * x_j)], sumqx += (w_j q) x_j, sumq2 += (w_j q) q in j order"""
    q = KVF[best_index((idv[:, None] * xb).astype(F))]
    sumqx = np.zeros(xb.shape[0], dtype=F)
    sumq2 = np.zeros(xb.shape[0], dtype=F)
    for j in range(32):
        wq = (w[:, j] * q[:, j]).astype(F)
        sumqx = (sumqx + (wq * xb[:, j]).astype(F)).astype(F)
        sumq2 = (sumq2 + (wq * q[:, j]).astype(F)).astype(F)
    return sumqx, sumq2


def block_scales(xb):
    """xb [nb, 32] f32 -> the scale of every block [nb] f32 (0 where amax < 1e-15f)"""
    xb = np.ascontiguousarray(xb, dtype=F).reshape(-1, 32)
    with np.errstate(over="ignore"):
        w = (xb * xb).astype(F)
    amax = np.zeros(xb.shape[0], dtype=F)
    mx = np.zeros(xb.shape[0], dtype=F)
    for j in range(32):                                                   # the FIRST element of largest magnitude (strict >, from 0)
        ax = np.abs(xb[:, j])
        take = ax > amax
        amax = np.where(take, ax, amax)
        mx = np.where(take, xb[:, j], mx)
    live = ~(amax < F(1e-15))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        d = ((-mx).astype(F) / KVF[0]).astype(F)
        sumqx, sumq2 = _sums(xb, w, (F(1) / d).astype(F))
        d = (sumqx / sumq2).astype(F)
        best = (d * sumqx).astype(F)
        for itry in range(-7, 8):
            sqx, sq2 = _sums(xb, w, (F(itry + int(KV[0])) / mx).astype(F))
            acc = (sq2 > 0) & ((sqx * sqx).astype(F) > (best * sq2).astype(F))
            dn = (sqx / sq2).astype(F)
            d = np.where(acc, dn, d).astype(F)
            best = np.where(acc, (dn * sqx).astype(F), best).astype(F)
    return np.where(live, d, F(0)).astype(F)


def _inv(v):
    with np.errstate(divide="ignore", over="ignore"):
        return np.where(v != 0, (F(1) / v).astype(F), F(0)).astype(F)


def quantize_iq4_nl(x):
    """x [..., K] f32 (K % 32 == 0) -> [nb, 18] blocks"""
    xb = np.ascontiguousarray(x, dtype=F).reshape(-1, 32)
    s = block_scales(xb)
    with np.errstate(over="ignore"):
        d16 = s.astype(np.float16)
    L = best_index((_inv(s)[:, None] * xb).astype(F))
    return pack_iq4_nl(L, d16)


def quantize_iq4_xs(x):
    """x [..., K] f32 (K % 256 == 0) -> [nb, 136] super-blocks"""
    xs = np.ascontiguousarray(x, dtype=F).reshape(-1, 8, 32)
    nsb = xs.shape[0]
    s = block_scales(xs.reshape(-1, 32)).reshape(nsb, 8)
    amax_s = np.zeros(nsb, dtype=F)
    max_scale = np.zeros(nsb, dtype=F)
    for ib in range(8):                                                   # the FIRST scale of largest magnitude (strict >, from 0)
        a = np.abs(s[:, ib])
        take = a > amax_s
        amax_s = np.where(take, a, amax_s)
        max_scale = np.where(take, s[:, ib], max_scale)
    D = ((-max_scale).astype(F) / F(32)).astype(F)
    d16 = D.astype(np.float16)
    iD = _inv(D)
    r = np.rint((iD[:, None] * s).astype(F))
    l = np.where(np.isnan(r), 0, np.clip(np.nan_to_num(r), -32, 31)).astype(np.int64)   # nearest(NaN) = 0 (a NaN scale: an overflowed fit)
    dl = (D[:, None] * l.astype(F)).astype(F)
    L = best_index((_inv(dl)[:, :, None] * xs).astype(F))
    return pack_iq4_xs(L, l + 32, d16)
