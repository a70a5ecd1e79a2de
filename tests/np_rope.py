"""numpy restatements for tests/test_rope.py: the per-pair constants of include/ggml_hip_ext.h's ROPE section in float64 (the yardstick of
ggml_hip_rope_table: no upstream source is at hand, so the header's text and this file are the definition, as for IQ4), the exact float64
rotation as REFERENCE, and a float32 MODEL of the statement the header writes down for the device.

  table       extrap_i = base^(-2i/n_dims); the YaRN ramp between the correction dims; eff_i = extrap_i (scale (1 - mix_i) + mix_i); mscale
  reference   theta = pos * eff_i [/ ff_i];  y0 = x0 cos(theta) mscale - x1 sin(theta) mscale,  y1 = x0 sin .. + x1 cos ..   all float64
  model       c = float32(cos(theta) * mscale), s = float32(sin(theta) * mscale) from the float64 angle; y0 = x0 * c - x1 * s and
              y1 = x0 * s + x1 * c with every float32 operation rounded once

The statistic of an element is  |y - ref| / (2^-24 * mscale * (|x0| + |x1|)).  The bar of the kernels is 4, DERIVED, not measured: one
rounding each for c (or s), for the product and for the sum make 3 units (each at most 2^-24 of a quantity bounded by mscale (|x0| + |x1|));
the fourth covers the table's slack at positions <= 2^20 (2^-48 relative * 2^20 rad = 2^-28 rad) and the device's libm.  The model's own
worst statistic on the sweep (cases()) is recorded as MODEL_WORST and recomputed on the CPU by
test_the_model_constant_is_what_the_model_measures."""
import numpy as np

NORMAL, NEOX = 0, 2
U = 2.0 ** -24
BAR = 4.0
MODEL_WORST = 2.7           # measured 2.30 (NORMAL) / 2.61 (NEOX) on the sweep, recorded rounded up; at most 3 by the derivation above


def params(n_dims, mode=NORMAL, freq_base=10000.0, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0, n_ctx_orig=0):
    """the parameter struct as a dict; the float fields carry binary32 values, as the C struct does"""
    f = lambda v: float(np.float32(v))
    return dict(n_dims=int(n_dims), mode=int(mode), n_ctx_orig=int(n_ctx_orig), freq_base=f(freq_base), freq_scale=f(freq_scale), ext_factor=f(ext_factor),
                attn_factor=f(attn_factor), beta_fast=f(beta_fast), beta_slow=f(beta_slow))


# the three parameter sets of the issue: plain, a large base with a scale, YaRN
PARAM_SETS = {
    "plain": dict(freq_base=10000.0, freq_scale=1.0),
    "scaled": dict(freq_base=500000.0, freq_scale=0.25),
    "yarn": dict(freq_base=10000.0, freq_scale=0.25, ext_factor=1.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0, n_ctx_orig=4096),
}


def table(p):
    """(eff float64 [n_dims / 2], mscale float64): the header's formulas"""
    n_dims, base, scale, ext = p["n_dims"], np.float64(p["freq_base"]), np.float64(p["freq_scale"]), np.float64(p["ext_factor"])
    i = np.arange(n_dims // 2, dtype=np.float64)
    extrap = base ** (-2.0 * i / n_dims)
    mix = np.zeros_like(i)
    mscale = np.float64(p["attn_factor"])
    if ext != 0.0:
        corr = lambda r: n_dims * np.log(p["n_ctx_orig"] / (2.0 * np.pi * np.float64(r))) / (2.0 * np.log(base))
        low = max(0.0, np.floor(corr(p["beta_fast"])))
        high = min(n_dims - 1.0, np.ceil(corr(p["beta_slow"])))
        ramp = 1.0 - np.clip((i - low) / max(0.001, high - low), 0.0, 1.0)
        mix = ramp * ext
        mscale = mscale * (1.0 + 0.1 * np.log(1.0 / scale))
    return extrap * (scale * (1.0 - mix) + mix), float(mscale)


def _pairs(p, D):
    """index arrays (e0, e1) of the rotated pairs of a row"""
    h = p["n_dims"] // 2
    i = np.arange(h)
    return (2 * i, 2 * i + 1) if p["mode"] == NORMAL else (i, i + h)


def _angles(p, pos, ff):
    eff, mscale = table(p)
    theta = np.asarray(pos, np.float64)[:, None] * eff[None, :]
    if ff is not None:
        theta = theta / np.asarray(ff, np.float32).astype(np.float64)[None, :]
    return theta, mscale


def reference(p, x, pos, ff=None):
    """x f32 [n_tokens, n_head, D], pos [n_tokens] -> float64 [n_tokens, n_head, D], the exact rotation; elements n_dims .. D-1 copied"""
    theta, mscale = _angles(p, pos, ff)
    e0, e1 = _pairs(p, x.shape[-1])
    c, s = (np.cos(theta) * mscale)[:, None, :], (np.sin(theta) * mscale)[:, None, :]
    x64 = np.asarray(x, np.float32).astype(np.float64)
    y = x64.copy()
    y[..., e0] = x64[..., e0] * c - x64[..., e1] * s
    y[..., e1] = x64[..., e0] * s + x64[..., e1] * c
    return y


def model(p, x, pos, ff=None):
    """the float32 statement of the header -> f32 [n_tokens, n_head, D]"""
    theta, mscale = _angles(p, pos, ff)
    e0, e1 = _pairs(p, x.shape[-1])
    c, s = (np.cos(theta) * mscale).astype(np.float32)[:, None, :], (np.sin(theta) * mscale).astype(np.float32)[:, None, :]
    x = np.asarray(x, np.float32)
    y = x.copy()
    x0, x1 = x[..., e0], x[..., e1]
    y[..., e0] = ((x0 * c).astype(np.float32) - (x1 * s).astype(np.float32)).astype(np.float32)
    y[..., e1] = ((x0 * s).astype(np.float32) + (x1 * c).astype(np.float32)).astype(np.float32)
    return y


def statistic(p, x, y, ref):
    """worst |y - ref| / (2^-24 mscale (|x0| + |x1|)) over the rotated elements; the copied ones must equal x bit for bit (else inf)"""
    _, mscale = table(p)
    e0, e1 = _pairs(p, x.shape[-1])
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    if not np.array_equal(y[..., p["n_dims"]:].view(np.uint32), x[..., p["n_dims"]:].view(np.uint32)):
        return float("inf")
    mag = (np.abs(x[..., e0]).astype(np.float64) + np.abs(x[..., e1]).astype(np.float64)) * mscale * U
    worst = 0.0
    for e in (e0, e1):
        err = np.abs(y[..., e].astype(np.float64) - ref[..., e])
        if np.any((mag == 0) & (err != 0)):
            return float("inf")
        worst = max(worst, float((err[mag > 0] / mag[mag > 0]).max(initial=0.0)))
    return worst


# ---- the sweep both the CPU model test and the GPU tests walk ----
SHAPES = ((64, 64), (128, 128), (128, 64), (64, 32), (12, 6))       # (D, n_dims); the last is the one-element-at-a-time path
MODES = (NORMAL, NEOX)
N_HEAD = (1, 4)
N_TOKENS = (1, 3, 130)
POSITIONS = (0, 1, 127, 128, 4095, (1 << 20) - 1)
SETS = ("plain", "scaled", "yarn", "ff")                           # "ff": the plain set with llama-3 style frequency factors


def cases(D=None, n_dims=None, mode=None):
    """(D, n_dims, mode, n_head, n_tokens, set name) of the sweep, optionally of one (D, n_dims, mode)"""
    out = []
    for sD, sn in SHAPES:
        for m in MODES:
            if (D, n_dims, mode) != (None, None, None) and (sD, sn, m) != (D, n_dims, mode):
                continue
            for nh in N_HEAD:
                for nt in N_TOKENS:
                    for name in SETS:
                        out.append((sD, sn, m, nh, nt, name))
    return out


def case_params(case):
    D, n_dims, mode, _, _, name = case
    return params(n_dims, mode, **PARAM_SETS["plain" if name == "ff" else name])


_INPUTS = {}


def inputs(case):
    """seeded (x f32 [n_tokens, n_head, D] in [-1, 1], pos int32 [n_tokens] walking POSITIONS with repeats, ff f32 [n_dims / 2] or None)"""
    if case not in _INPUTS:
        D, n_dims, mode, n_head, n_tokens, name = case
        k = SETS.index(name)
        rng = np.random.default_rng([D, n_dims, mode, n_head, n_tokens, k])
        x = rng.uniform(-1, 1, (n_tokens, n_head, D)).astype(np.float32)
        start = (k + n_head + D + n_dims + mode) % len(POSITIONS)
        pos = np.array([POSITIONS[(start + t) % len(POSITIONS)] for t in range(n_tokens)], np.int32)
        ff = rng.uniform(1.0, 8.0, n_dims // 2).astype(np.float32) if name == "ff" else None
        _INPUTS[case] = (x, pos, ff)
    return _INPUTS[case]


_REFS = {}


def case_reference(case):
    if case not in _REFS:
        x, pos, ff = inputs(case)
        _REFS[case] = reference(case_params(case), x, pos, ff)
    return _REFS[case]
