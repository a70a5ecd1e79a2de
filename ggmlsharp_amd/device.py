"""Device-level helpers over the C-ABI: resident weights and the hot path on HBM-resident buffers.

torch is used for device memory and streams only (torch tensors own the buffers; the kernels are ours and run on
torch's current stream).  Nothing here computes on the CPU.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, row_bytes


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def init(device=None):
    if device is None:
        device = torch.cuda.current_device()
    check(lib().ggml_hip_init(int(device)), "ggml_hip_init")


class Weight:
    """One resident 2-D weight matrix [M rows, K] (a row shard when row_begin/row_end are given)."""

    def __init__(self, handle, type, M, K):
        self.handle, self.type, self.M, self.K = handle, type, M, K

    @staticmethod
    def row_bytes(type, K):
        return row_bytes(type, K)

    @classmethod
    def from_host(cls, type, rows, K, row_begin=0, row_end=None):
        """rows: numpy uint8/f32/f16 array holding M reference-format rows (contiguous)."""
        rows = np.ascontiguousarray(rows)
        rb = cls.row_bytes(type, K)
        M = rows.nbytes // rb
        if row_end is None:
            row_end = M
        h = C.c_void_p()
        check(lib().ggml_hip_weight_upload(type, rows.ctypes.data_as(C.c_void_p), K, M, rb, row_begin, row_end,
                                           _stream(), C.byref(h)), "ggml_hip_weight_upload")
        return cls(h, type, row_end - row_begin, K)

    @classmethod
    def from_device(cls, type, rows_t, K, row_begin=0, row_end=None):
        rb = cls.row_bytes(type, K)
        M = rows_t.numel() * rows_t.element_size() // rb
        if row_end is None:
            row_end = M
        h = C.c_void_p()
        check(lib().ggml_hip_weight_from_device(type, C.c_void_p(rows_t.data_ptr()), K, M, rb, row_begin, row_end,
                                                _stream(), C.byref(h)), "ggml_hip_weight_from_device")
        return cls(h, type, row_end - row_begin, K)

    def download(self):
        out = np.zeros(self.M * self.row_bytes(self.type, self.K), dtype=np.uint8)
        check(lib().ggml_hip_weight_download(self.handle, out.ctypes.data_as(C.c_void_p), _stream()),
              "ggml_hip_weight_download")
        return out

    def free(self):
        if self.handle:
            lib().ggml_hip_weight_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def work_size(type, K, N):
    return int(lib().ggml_hip_mul_mat_work_size(type, K, N))


def alloc_work(type, K, N, device=None):
    n = max(work_size(type, K, N), 16)
    return torch.empty(n, dtype=torch.uint8, device=device or "cuda")


def mul_mat(w, x, out=None, work=None):
    """dst[N, M] = mul_mat(w, x[N, K]) on the current stream; x f32 row-major on the device."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    N = x.shape[0]
    if out is None:
        out = torch.empty((N, w.M), dtype=torch.float32, device=x.device)
    if work is None:
        work = alloc_work(w.type, w.K, N, x.device)
    check(lib().ggml_hip_mul_mat_dev(w.handle, C.c_void_p(x.data_ptr()), N, x.stride(0), C.c_void_p(out.data_ptr()),
                                     out.stride(0), C.c_void_p(work.data_ptr()), work.numel(), _stream()),
          "ggml_hip_mul_mat_dev")
    return out


def mul_mat_init(w, x, work):
    check(lib().ggml_hip_mul_mat_init_dev(w.handle, C.c_void_p(x.data_ptr()), x.shape[0], x.stride(0),
                                          C.c_void_p(work.data_ptr()), work.numel(), _stream()),
          "ggml_hip_mul_mat_init_dev")


def mul_mat_compute(w, N, out, work):
    check(lib().ggml_hip_mul_mat_compute_dev(w.handle, N, C.c_void_p(out.data_ptr()), out.stride(0),
                                             C.c_void_p(work.data_ptr()), work.numel(), _stream()),
          "ggml_hip_mul_mat_compute_dev")


class ExpertSet:
    """The experts of one mixture-of-experts projection: 2 .. 1024 resident weights of one type and shape on one device.  The set keeps the
    Weight objects alive (the library's set does not own them)."""

    def __init__(self, weights):
        self.weights = list(weights)
        self.M, self.K, self.type = self.weights[0].M, self.weights[0].K, self.weights[0].type
        hw = (C.c_void_p * len(self.weights))(*[w.handle for w in self.weights])
        h = C.c_void_p()
        check(lib().ggml_hip_expert_set_create(hw, len(self.weights), _stream(), C.byref(h)), "ggml_hip_expert_set_create")
        self.handle = h

    def route(self, n_tokens, n_used):
        return int(lib().ggml_hip_mul_mat_id_route(self.handle, n_tokens, n_used))

    def work_size(self, n_tokens, n_used):
        return int(lib().ggml_hip_mul_mat_id_work_size(self.handle, n_tokens, n_used))

    def grouped_serves(self):
        return int(lib().ggml_hip_mul_mat_id_grouped_serves(self.handle))

    def grouped_work_size(self, n_tokens, n_used):
        return int(lib().ggml_hip_mul_mat_id_grouped_work_size(self.handle, n_tokens, n_used))

    def free(self):
        if self.handle:
            lib().ggml_hip_expert_set_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def mul_mat_id(es, ids, x, h_ids=None, out=None, work=None):
    """dst[n_tokens, n_used, M]: pair (t, s) = expert ids[t, s] of the set against its src1 row, on the current stream.
    ids int32 [n_tokens, n_used] on the device; x f32 [n_tokens, K] (one row per token, upstream's broadcast) or [n_tokens, n_used, K];
    h_ids: the same ids as a numpy int32 array (the batch route then runs without a synchronize)."""
    assert ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 2 and ids.is_contiguous()
    assert x.is_cuda and x.dtype == torch.float32 and x.stride(-1) == 1 and x.shape[0] == ids.shape[0]
    n_tokens, n_used = ids.shape
    ld1_slot = 0 if x.dim() == 2 else x.stride(1)
    if out is None:
        out = torch.empty((n_tokens, n_used, es.M), dtype=torch.float32, device=x.device)
    if work is None:
        work = torch.empty(max(es.work_size(n_tokens, n_used), 16), dtype=torch.uint8, device=x.device)
    hp = None
    if h_ids is not None:
        h_ids = np.ascontiguousarray(h_ids, dtype=np.int32)
        assert h_ids.size == n_tokens * n_used
        hp = h_ids.ctypes.data_as(C.c_void_p)
    check(lib().ggml_hip_mul_mat_id_dev(es.handle, C.c_void_p(ids.data_ptr()), hp, n_tokens, n_used, C.c_void_p(x.data_ptr()), x.stride(0), ld1_slot,
                                        C.c_void_p(out.data_ptr()), out.stride(1), C.c_void_p(work.data_ptr()), work.numel(), _stream()),
          "ggml_hip_mul_mat_id_dev")
    return out


def mul_mat_id_grouped(es, ids, x, out=None, work=None):
    """mul_mat_id's result through the grouped route: the ids are read on the device alone, the launches do not depend on them (capturable;
    a replay follows the ids it finds).  Arguments as mul_mat_id's, without h_ids; the set must be served (es.grouped_serves())."""
    assert ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 2 and ids.is_contiguous()
    assert x.is_cuda and x.dtype == torch.float32 and x.stride(-1) == 1 and x.shape[0] == ids.shape[0]
    n_tokens, n_used = ids.shape
    ld1_slot = 0 if x.dim() == 2 else x.stride(1)
    if out is None:
        out = torch.empty((n_tokens, n_used, es.M), dtype=torch.float32, device=x.device)
    if work is None:
        work = torch.empty(max(es.grouped_work_size(n_tokens, n_used), 16), dtype=torch.uint8, device=x.device)
    check(lib().ggml_hip_mul_mat_id_grouped_dev(es.handle, C.c_void_p(ids.data_ptr()), n_tokens, n_used, C.c_void_p(x.data_ptr()), x.stride(0), ld1_slot,
                                                C.c_void_p(out.data_ptr()), out.stride(1), C.c_void_p(work.data_ptr()), work.numel(), _stream()),
          "ggml_hip_mul_mat_id_grouped_dev")
    return out


def moe_route(logits, n_used, gating=0, normalize=True, scale=1.0, ids=None, weights=None):
    """router logits f32 [n_tokens, n_expert] on the device (row stride may exceed n_expert) -> (ids int32, weights f32), both
    [n_tokens, n_used]: the n_used largest logits of a token in rank order (ties: the smaller index) and their gate weights
    (gating 0 softmax over all experts, 1 sigmoid; normalize: over the selected ones; then * scale).  On the current stream."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    n_tokens, n_expert = logits.shape
    if ids is None:
        ids = torch.empty((n_tokens, n_used), dtype=torch.int32, device=logits.device)
    if weights is None:
        weights = torch.empty((n_tokens, n_used), dtype=torch.float32, device=logits.device)
    assert ids.is_contiguous() and weights.is_contiguous() and ids.dtype == torch.int32 and weights.dtype == torch.float32
    check(lib().ggml_hip_moe_route_dev(C.c_void_p(logits.data_ptr()), logits.stride(0), n_tokens, n_expert, n_used, int(gating), int(bool(normalize)),
                                       float(scale), C.c_void_p(ids.data_ptr()), C.c_void_p(weights.data_ptr()), _stream()), "ggml_hip_moe_route_dev")
    return ids, weights


def moe_combine(y, weights, addend=None, out=None):
    """out[t] = sum over the slots s (ascending) of weights[t, s] * y[t, s] (+ addend[t]): y f32 [n_tokens, n_used, M] as the mul_mat_id
    entries write it, weights f32 [n_tokens, n_used]; out may be addend itself.  On the current stream."""
    assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 3 and y.stride(2) == 1 and y.stride(0) == y.shape[1] * y.stride(1)
    assert weights.is_cuda and weights.dtype == torch.float32 and weights.is_contiguous() and tuple(weights.shape) == tuple(y.shape[:2])
    n_tokens, n_used, M = y.shape
    if out is None:
        out = torch.empty((n_tokens, M), dtype=torch.float32, device=y.device)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1
    ap, ld_add = None, 0
    if addend is not None:
        assert addend.is_cuda and addend.dtype == torch.float32 and addend.dim() == 2 and addend.stride(1) == 1
        ap, ld_add = C.c_void_p(addend.data_ptr()), addend.stride(0)
    check(lib().ggml_hip_moe_combine_dev(C.c_void_p(y.data_ptr()), y.stride(1), C.c_void_p(weights.data_ptr()), n_tokens, n_used, M, ap, ld_add,
                                         C.c_void_p(out.data_ptr()), out.stride(0), _stream()), "ggml_hip_moe_combine_dev")
    return out


def silu_mul_rows(a, b, silu=None, out=None):
    """out = silu(a) * b on contiguous f32 rows (the SwiGLU pair, the reference's GGML_SILU_FP16 form); silu, when given, receives silu(a)."""
    assert a.is_cuda and b.is_cuda and a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and a.shape == b.shape
    if out is None:
        out = torch.empty_like(a)
    assert out.is_contiguous() and (silu is None or silu.is_contiguous())
    k = a.shape[-1] if a.dim() else 1
    check(lib().ggml_hip_silu_mul_rows_dev(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(silu.data_ptr()) if silu is not None else None,
                                           C.c_void_p(out.data_ptr()), a.numel() // max(k, 1), k, _stream()), "ggml_hip_silu_mul_rows_dev")
    return out


def kv_row_bytes(kv_type, D):
    """bytes of one cache row of D elements (F16 or Q8_0) in reference block format"""
    return row_bytes(kv_type, D)


def kv_store(kv_type, x, cache, nb_pos, n_pos_max, pos0=0, d_pos0=None):
    """append rows to a KV cache: x f32 [n_rows, row_elems] on the device (row stride a multiple of 4) -> rows of kv_type (F16 / Q8_0) at
    cache + (pos0 + i) * nb_pos bytes; cache: a uint8 tensor whose first byte is position 0 (a view selects a head of a head-major cache).
    d_pos0: an int32 tensor on the device read instead of pos0 (a captured call follows it).  Positions outside [0, n_pos_max) write nothing."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    assert cache.is_cuda and cache.dtype == torch.uint8
    assert d_pos0 is None or (d_pos0.is_cuda and d_pos0.dtype == torch.int32)
    n_rows, row_elems = x.shape
    check(lib().ggml_hip_kv_store_dev(kv_type, C.c_void_p(x.data_ptr()), x.stride(0), n_rows, row_elems, C.c_void_p(cache.data_ptr()), nb_pos, n_pos_max,
                                      int(pos0), C.c_void_p(d_pos0.data_ptr()) if d_pos0 is not None else None, _stream()), "ggml_hip_kv_store_dev")


def attn_plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max):
    """(form, chunk, q_tile, launches, n_chunks, workgroups) of one attention call: form 1 DECODE, 2 PROMPT (0 for n_q = 0); no device needed"""
    out = _lib.ggml_hip_attn_plan_t()
    check(lib().ggml_hip_attn_plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, C.byref(out)), "ggml_hip_attn_plan")
    return out


def attn_work_size(kv_type, D, n_head, n_head_kv, n_q, n_kv_max):
    return int(lib().ggml_hip_attn_work_size(kv_type, D, n_head, n_head_kv, n_q, n_kv_max))


def attn_opts(window=0, softcap=0.0, sinks=None):
    """a ggml_hip_attn_opts_t (sinks: an f32 tensor [n_head] on the device, kept alive by the caller), or None when every option is off"""
    if not window and not softcap and sinks is None:
        return None
    assert sinks is None or (sinks.is_cuda and sinks.dtype == torch.float32 and sinks.is_contiguous())
    return _lib.ggml_hip_attn_opts_t(sinks.data_ptr() if sinks is not None else None, int(window), float(softcap), 0)


def alibi_slopes(n_head, max_bias):
    """upstream's ALiBi slopes of n_head heads as a numpy f32 vector (ggml_hip_alibi_slopes: host only; max_bias 0 gives ones); upload it for slopes="""
    out = np.empty(n_head, np.float32)
    check(lib().ggml_hip_alibi_slopes(int(n_head), float(max_bias), out.ctypes.data_as(C.c_void_p)), "ggml_hip_alibi_slopes")
    return out


def attn_bias(mask=None, slopes=None):
    """a ggml_hip_attn_bias_t, or None without a mask and slopes.  mask: an f16 tensor [rows, >= n_kv_max] on the device, last stride 1, row stride a
    multiple of 8, row = the query's row index in q, column = the position (-inf: hidden; else added to the score times the head's slope); slopes:
    f32 [n_head] on the device.  Both are kept alive by the caller."""
    if mask is None and slopes is None:
        return None
    if mask is not None:
        assert mask.is_cuda and mask.dtype == torch.float16 and mask.dim() == 2 and mask.stride(1) == 1
    if slopes is not None:
        assert slopes.is_cuda and slopes.dtype == torch.float32 and slopes.is_contiguous()
    return _lib.ggml_hip_attn_bias_t(mask.data_ptr() if mask is not None else None, mask.stride(0) if mask is not None else 0,
                                     slopes.data_ptr() if slopes is not None else None)


def attn_ex_plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, window=0, softcap=0.0):
    """attn_plan under the options: a windowed DECODE call has min(ceil(n_kv_max / 128), ceil((window + n_q - 1) / 128) + 1) chunks; no device needed"""
    out = _lib.ggml_hip_attn_plan_t()
    opts = _lib.ggml_hip_attn_opts_t(None, int(window), float(softcap), 0)
    check(lib().ggml_hip_attn_ex_plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, C.byref(opts), C.byref(out)), "ggml_hip_attn_ex_plan")
    return out


def attention(kv_type, q, k, v, nb_pos, nb_head, n_head_kv, n_kv, d_n_kv=None, n_kv_max=None, causal=True, scale=None, out=None, work=None, window=0,
              softcap=0.0, sinks=None, mask=None, slopes=None):
    """out[t, h] = softmax_j(scale * q[t, h] . K[j, h / G]) V[j, h / G] over the visible j of an F16 / Q8_0 cache, on the current stream.
    q f32 [n_q, n_head, D] (last stride 1); k, v: uint8 tensors whose first byte is row (position 0, kv head 0), rows nb_pos / nb_head bytes
    apart; causal: the batch is the last n_q of the n_kv positions.  d_n_kv: an int32 tensor on the device read instead of n_kv (clamped to
    n_kv_max, which sizes the launch; default n_kv).  scale defaults to 1 / sqrt(D).
    window (0: none; W: a row at position P sees j with P - j < W), softcap (0: none) and sinks (f32 [n_head] on the device) go through
    ggml_hip_attn_ex_dev; with all three off the call is ggml_hip_attn_dev as before.
    mask (f16 [n_q, >= n_kv_max] on the device: -inf hides position j from row t, any other value is added to the score times the head's slope) and
    slopes (f32 [n_head] on the device, alibi_slopes) go through ggml_hip_attn_bias_dev, with the options."""
    assert q.is_cuda and q.dtype == torch.float32 and q.dim() == 3 and q.stride(2) == 1
    assert k.is_cuda and v.is_cuda and k.dtype == torch.uint8 and v.dtype == torch.uint8
    assert d_n_kv is None or (d_n_kv.is_cuda and d_n_kv.dtype == torch.int32)
    n_q, n_head, D = q.shape
    if n_kv_max is None:
        n_kv_max = n_kv
    if scale is None:
        scale = 1.0 / float(np.sqrt(np.float64(D)))
    if out is None:
        out = torch.empty((n_q, n_head, D), dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and out.dim() == 3 and out.stride(2) == 1 and tuple(out.shape) == (n_q, n_head, D)
    if work is None:
        work = torch.empty(max(attn_work_size(kv_type, D, n_head, n_head_kv, n_q, n_kv_max), 16), dtype=torch.uint8, device=q.device)
    opts = attn_opts(window, softcap, sinks)
    bias = attn_bias(mask, slopes)
    if bias is not None:
        check(lib().ggml_hip_attn_bias_dev(kv_type, C.c_void_p(q.data_ptr()), q.stride(0), q.stride(1), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), nb_pos,
                                           nb_head, n_head, n_head_kv, D, n_q, int(n_kv), C.c_void_p(d_n_kv.data_ptr()) if d_n_kv is not None else None, n_kv_max,
                                           int(bool(causal)), float(scale), C.byref(opts) if opts is not None else None, C.byref(bias),
                                           C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1), C.c_void_p(work.data_ptr()), work.numel(), _stream()),
              "ggml_hip_attn_bias_dev")
        return out
    if opts is not None:
        check(lib().ggml_hip_attn_ex_dev(kv_type, C.c_void_p(q.data_ptr()), q.stride(0), q.stride(1), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), nb_pos,
                                         nb_head, n_head, n_head_kv, D, n_q, int(n_kv), C.c_void_p(d_n_kv.data_ptr()) if d_n_kv is not None else None, n_kv_max,
                                         int(bool(causal)), float(scale), C.byref(opts), C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1),
                                         C.c_void_p(work.data_ptr()), work.numel(), _stream()), "ggml_hip_attn_ex_dev")
        return out
    check(lib().ggml_hip_attn_dev(kv_type, C.c_void_p(q.data_ptr()), q.stride(0), q.stride(1), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), nb_pos, nb_head,
                                  n_head, n_head_kv, D, n_q, int(n_kv), C.c_void_p(d_n_kv.data_ptr()) if d_n_kv is not None else None, n_kv_max,
                                  int(bool(causal)), float(scale), None, 0.0, 0.0, None, C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1),
                                  C.c_void_p(work.data_ptr()), work.numel(), _stream()), "ggml_hip_attn_dev")
    return out


def rope_params(n_dims, mode=0, freq_base=10000.0, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0, n_ctx_orig=0):
    """a ggml_hip_rope_params_t: mode 0 NORMAL (pairs 2i, 2i+1), 2 NEOX (pairs i, i + n_dims/2); ext_factor != 0 turns YaRN on"""
    return _lib.ggml_hip_rope_params_t(int(n_dims), int(mode), int(n_ctx_orig), float(freq_base), float(freq_scale), float(ext_factor), float(attn_factor),
                                       float(beta_fast), float(beta_slow))


def rope_table(rp):
    """(eff float64 [n_dims/2], mscale): the per-pair constants every rope kernel uses, as include/ggml_hip_ext.h defines them; no device needed"""
    eff = np.zeros(rp.n_dims // 2 if rp.n_dims > 0 else 0, dtype=np.float64)
    mscale = C.c_double()
    check(lib().ggml_hip_rope_table(C.byref(rp), eff.ctypes.data_as(C.POINTER(C.c_double)), C.byref(mscale)), "ggml_hip_rope_table")
    return eff, mscale.value


def _opt(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def rope(rp, x, pos=None, pos0=0, d_pos0=None, freq_factors=None, out=None):
    """rotate the rows of x f32 [n_tokens, n_head, D] (last stride 1) on the current stream.  Token t sits at pos[t] (an int32 tensor on the
    device), else at p0 + t with p0 = *d_pos0 (an int32 tensor on the device, read by the kernel) or pos0.  freq_factors: f32 [n_dims/2] on the
    device.  out may be x itself (in place); default a new tensor."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.stride(2) == 1
    assert pos is None or (pos.is_cuda and pos.dtype == torch.int32 and pos.is_contiguous() and pos.numel() == x.shape[0])
    assert d_pos0 is None or (d_pos0.is_cuda and d_pos0.dtype == torch.int32)
    assert freq_factors is None or (freq_factors.is_cuda and freq_factors.dtype == torch.float32 and freq_factors.is_contiguous())
    n_tokens, n_head, D = x.shape
    if out is None:
        out = torch.empty((n_tokens, n_head, D), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.dim() == 3 and out.stride(2) == 1 and tuple(out.shape) == (n_tokens, n_head, D)
    check(lib().ggml_hip_rope_dev(C.byref(rp), C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), n_head, D, n_tokens, _opt(pos), int(pos0), _opt(d_pos0),
                                  _opt(freq_factors), C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1), _stream()), "ggml_hip_rope_dev")
    return out


def rope_kv_store(rp, kv_type, x, cache, nb_pos, nb_head, n_pos_max, pos0=0, d_pos0=None, freq_factors=None):
    """rotate the rows of x f32 [n_tokens, n_head_kv, D] and store them as rows of kv_type (F16 / Q8_0) at cache + (p0 + t) * nb_pos +
    hk * nb_head bytes in one launch: bit for bit rope() into a temporary, then kv_store().  The rope position is the cache position p0 + t,
    p0 = *d_pos0 or pos0; positions outside [0, n_pos_max) write nothing."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.stride(2) == 1
    assert cache.is_cuda and cache.dtype == torch.uint8
    assert d_pos0 is None or (d_pos0.is_cuda and d_pos0.dtype == torch.int32)
    assert freq_factors is None or (freq_factors.is_cuda and freq_factors.dtype == torch.float32 and freq_factors.is_contiguous())
    n_tokens, n_head_kv, D = x.shape
    check(lib().ggml_hip_rope_kv_store_dev(C.byref(rp), kv_type, C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), n_head_kv, D, n_tokens, _opt(freq_factors),
                                           C.c_void_p(cache.data_ptr()), nb_pos, nb_head, n_pos_max, int(pos0), _opt(d_pos0), _stream()),
          "ggml_hip_rope_kv_store_dev")


class PagedCache:
    """how a paged KV cache is addressed (include/ggml_hip_ext.h, PAGED ATTENTION): pools k / v (uint8 tensors of n_pages pages of 128 positions,
    nb_page bytes apart; row (jj, hk) of a page at jj * nb_pos + hk * nb_head), the page table pages int32 [n_seq, ld_pages] and the lengths
    d_len int32 [n_seq] on the device, and n_kv_max, which sizes the launches (size it to the step).  The host owns the table."""

    def __init__(self, kv_type, k, v, nb_page, nb_pos, nb_head, n_pages, pages, d_len, n_kv_max):
        assert k.is_cuda and v.is_cuda and k.dtype == torch.uint8 and v.dtype == torch.uint8
        assert pages.is_cuda and pages.dtype == torch.int32 and pages.dim() == 2 and pages.stride(1) == 1
        assert d_len.is_cuda and d_len.dtype == torch.int32 and d_len.is_contiguous() and d_len.numel() == pages.shape[0]
        self.kv_type, self.k, self.v, self.nb_page, self.nb_pos, self.nb_head = kv_type, k, v, int(nb_page), int(nb_pos), int(nb_head)
        self.n_pages, self.pages, self.d_len, self.n_kv_max = int(n_pages), pages, d_len, int(n_kv_max)

    @property
    def n_seq(self):
        return self.pages.shape[0]

    def _args(self):
        """(nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len) as the entries take them"""
        return (self.nb_page, self.nb_pos, self.nb_head, self.n_pages, C.c_void_p(self.pages.data_ptr()), self.pages.stride(0), C.c_void_p(self.d_len.data_ptr()))


def _paged_rows(pc, x):
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.stride(2) == 1
    n_rows, n_head_kv, D = x.shape
    assert n_rows % pc.n_seq == 0, "n_seq * n_q rows"
    return n_rows // pc.n_seq, n_head_kv, D


def kv_store_paged(pc, x, pool):
    """x f32 [n_seq * n_q, n_head_kv, D] -> row (b, t, hk) to its page row of pool (pc.k or pc.v) at position d_len[b] + t, bit for bit
    kv_store's bytes; a position outside [0, n_kv_max) or a page id outside [0, n_pages) writes nothing"""
    n_q, n_head_kv, D = _paged_rows(pc, x)
    nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len = pc._args()
    check(lib().ggml_hip_kv_store_paged_dev(pc.kv_type, C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), n_head_kv, D, pc.n_seq, n_q, C.c_void_p(pool.data_ptr()),
                                            nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len, pc.n_kv_max, _stream()), "ggml_hip_kv_store_paged_dev")


def rope_kv_store_paged(rp, pc, x, pool, freq_factors=None):
    """rotate the rows of x f32 [n_seq * n_q, n_head_kv, D] at their cache positions d_len[b] + t and store them as page rows of pool in one
    launch: bit for bit rope(pos = d_len[b] + t) into a temporary, then kv_store_paged()"""
    assert freq_factors is None or (freq_factors.is_cuda and freq_factors.dtype == torch.float32 and freq_factors.is_contiguous())
    n_q, n_head_kv, D = _paged_rows(pc, x)
    nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len = pc._args()
    check(lib().ggml_hip_rope_kv_store_paged_dev(C.byref(rp), pc.kv_type, C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), n_head_kv, D, pc.n_seq, n_q,
                                                 _opt(freq_factors), C.c_void_p(pool.data_ptr()), nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len, pc.n_kv_max,
                                                 _stream()), "ggml_hip_rope_kv_store_paged_dev")


def attn_paged_plan(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max):
    """the ggml_hip_attn_plan_t of one paged call: attn_plan's form and chunk for n_q, the workgroups of all n_seq sequences; no device needed"""
    out = _lib.ggml_hip_attn_plan_t()
    check(lib().ggml_hip_attn_paged_plan(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, C.byref(out)), "ggml_hip_attn_paged_plan")
    return out


def attn_paged_work_size(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max):
    return int(lib().ggml_hip_attn_paged_work_size(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max))


def attn_paged_ex_plan(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, window=0, softcap=0.0):
    """attn_paged_plan under the options: attn_ex_plan's chunk count, the workgroups of all n_seq sequences; no device needed"""
    out = _lib.ggml_hip_attn_plan_t()
    opts = _lib.ggml_hip_attn_opts_t(None, int(window), float(softcap), 0)
    check(lib().ggml_hip_attn_paged_ex_plan(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, C.byref(opts), C.byref(out)), "ggml_hip_attn_paged_ex_plan")
    return out


def attn_paged(pc, q, n_head_kv, len_bias=0, causal=True, scale=None, out=None, work=None, window=0, softcap=0.0, sinks=None, mask=None, slopes=None):
    """attention of n_seq independent sequences over the paged cache pc in one call: q f32 [n_seq * n_q, n_head, D] (last stride 1), sequence b
    over its n_kv[b] = clamp(d_len[b] + len_bias, 0, n_kv_max) positions; its rows are bit for bit attention() on a contiguous copy of its cache.
    len_bias = n_q behind a store of this step's tokens.  A sequence with n_kv 0 or an invalid needed page id returns +0.0 rows.
    window, softcap, sinks: as attention(), through ggml_hip_attn_paged_ex_dev; under a window the table entries below a sequence's first
    needed chunk are never read (the host may recycle those pages).
    mask (f16 [n_seq * n_q, >= n_kv_max], row = the row of q, column = the position in that row's own sequence) and slopes: as attention(), through
    ggml_hip_attn_paged_bias_dev."""
    assert q.is_cuda and q.dtype == torch.float32 and q.dim() == 3 and q.stride(2) == 1
    n_rows, n_head, D = q.shape
    assert n_rows % pc.n_seq == 0, "n_seq * n_q rows"
    n_q = n_rows // pc.n_seq
    if scale is None:
        scale = 1.0 / float(np.sqrt(np.float64(D)))
    if out is None:
        out = torch.empty((n_rows, n_head, D), dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and out.dim() == 3 and out.stride(2) == 1 and tuple(out.shape) == (n_rows, n_head, D)
    if work is None:
        work = torch.empty(max(attn_paged_work_size(pc.kv_type, D, n_head, n_head_kv, pc.n_seq, n_q, pc.n_kv_max), 16), dtype=torch.uint8, device=q.device)
    nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len = pc._args()
    opts = attn_opts(window, softcap, sinks)
    bias = attn_bias(mask, slopes)
    if bias is not None:
        check(lib().ggml_hip_attn_paged_bias_dev(pc.kv_type, C.c_void_p(q.data_ptr()), q.stride(0), q.stride(1), C.c_void_p(pc.k.data_ptr()),
                                                 C.c_void_p(pc.v.data_ptr()), nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len, int(len_bias), pc.n_seq, n_head,
                                                 n_head_kv, D, n_q, pc.n_kv_max, int(bool(causal)), float(scale), C.byref(opts) if opts is not None else None,
                                                 C.byref(bias), C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1), C.c_void_p(work.data_ptr()),
                                                 work.numel(), _stream()), "ggml_hip_attn_paged_bias_dev")
        return out
    if opts is not None:
        check(lib().ggml_hip_attn_paged_ex_dev(pc.kv_type, C.c_void_p(q.data_ptr()), q.stride(0), q.stride(1), C.c_void_p(pc.k.data_ptr()),
                                               C.c_void_p(pc.v.data_ptr()), nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len, int(len_bias), pc.n_seq, n_head,
                                               n_head_kv, D, n_q, pc.n_kv_max, int(bool(causal)), float(scale), C.byref(opts), C.c_void_p(out.data_ptr()),
                                               out.stride(0), out.stride(1), C.c_void_p(work.data_ptr()), work.numel(), _stream()), "ggml_hip_attn_paged_ex_dev")
        return out
    check(lib().ggml_hip_attn_paged_dev(pc.kv_type, C.c_void_p(q.data_ptr()), q.stride(0), q.stride(1), C.c_void_p(pc.k.data_ptr()), C.c_void_p(pc.v.data_ptr()),
                                        nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len, int(len_bias), pc.n_seq, n_head, n_head_kv, D, n_q, pc.n_kv_max,
                                        int(bool(causal)), float(scale), None, 0.0, 0.0, None, C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1),
                                        C.c_void_p(work.data_ptr()), work.numel(), _stream()), "ggml_hip_attn_paged_dev")
    return out


MLA_DK, MLA_DV = 576, 512


def attn_mla_plan(kv_type, n_head, n_q, n_kv_max, n_seq=None):
    """the ggml_hip_attn_mla_plan_t of one MLA call (n_seq: the paged call): form 1 SPLIT (n_q <= 8), 2 WALK; span = MLA_SPAN chunks of 128 positions per
    partial; n_spans, workgroups, merge_workgroups, work_bytes; no device needed"""
    out = _lib.ggml_hip_attn_mla_plan_t()
    if n_seq is None:
        check(lib().ggml_hip_attn_mla_plan(kv_type, MLA_DK, MLA_DV, n_head, n_q, n_kv_max, C.byref(out)), "ggml_hip_attn_mla_plan")
    else:
        check(lib().ggml_hip_attn_mla_paged_plan(kv_type, MLA_DK, MLA_DV, n_head, n_seq, n_q, n_kv_max, C.byref(out)), "ggml_hip_attn_mla_paged_plan")
    return out


def attn_mla_work_size(kv_type, n_head, n_q, n_kv_max, n_seq=None):
    if n_seq is None:
        return int(lib().ggml_hip_attn_mla_work_size(kv_type, MLA_DK, MLA_DV, n_head, n_q, n_kv_max))
    return int(lib().ggml_hip_attn_mla_paged_work_size(kv_type, MLA_DK, MLA_DV, n_head, n_seq, n_q, n_kv_max))


def attention_mla(kv_type, q, cache, nb_pos, n_kv, scale, d_n_kv=None, n_kv_max=None, causal=True, out=None, work=None):
    """MLA in the absorbed form: out[t, h] = softmax_j(scale * q[t, h] . row_j) row_j[:512] over the visible j of a latent cache, on the current stream.
    q f32 [n_q, n_head, 576] (last stride 1); cache: a uint8 tensor whose first byte is position 0, ONE row of 576 elements (F16 / Q8_0) per position,
    nb_pos bytes apart, shared by every head: columns 0 .. 511 are the latent and the value, 512 .. 575 the rotated key part.  scale is required (MLA's is
    not 1 / sqrt(576)).  d_n_kv, n_kv_max, causal: as attention().  Returns f32 [n_q, n_head, 512]."""
    assert q.is_cuda and q.dtype == torch.float32 and q.dim() == 3 and q.stride(2) == 1 and q.shape[2] == MLA_DK
    assert cache.is_cuda and cache.dtype == torch.uint8
    assert d_n_kv is None or (d_n_kv.is_cuda and d_n_kv.dtype == torch.int32)
    n_q, n_head, _ = q.shape
    if n_kv_max is None:
        n_kv_max = n_kv
    if out is None:
        out = torch.empty((n_q, n_head, MLA_DV), dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and out.dim() == 3 and out.stride(2) == 1 and tuple(out.shape) == (n_q, n_head, MLA_DV)
    if work is None:
        work = torch.empty(max(attn_mla_work_size(kv_type, n_head, n_q, n_kv_max), 16), dtype=torch.uint8, device=q.device)
    check(lib().ggml_hip_attn_mla_dev(kv_type, C.c_void_p(q.data_ptr()), q.stride(0), q.stride(1), C.c_void_p(cache.data_ptr()), nb_pos, n_head, MLA_DK, MLA_DV, n_q,
                                      int(n_kv), _opt(d_n_kv), n_kv_max, int(bool(causal)), float(scale), C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1),
                                      C.c_void_p(work.data_ptr()), work.numel(), _stream()), "ggml_hip_attn_mla_dev")
    return out


class LatentCache:
    """how a paged LATENT cache is addressed (include/ggml_hip_ext.h, MLA): one pool (a uint8 tensor of n_pages pages of 128 positions, nb_page bytes apart;
    the row of position jj of a page at jj * nb_pos, 576 elements of kv_type), the page table pages int32 [n_seq, ld_pages] and the lengths d_len int32
    [n_seq] on the device, and n_kv_max, which sizes the launches.  The host owns the table."""

    def __init__(self, kv_type, pool, nb_page, nb_pos, n_pages, pages, d_len, n_kv_max):
        assert pool.is_cuda and pool.dtype == torch.uint8
        assert pages.is_cuda and pages.dtype == torch.int32 and pages.dim() == 2 and pages.stride(1) == 1
        assert d_len.is_cuda and d_len.dtype == torch.int32 and d_len.is_contiguous() and d_len.numel() == pages.shape[0]
        self.kv_type, self.pool, self.nb_page, self.nb_pos = kv_type, pool, int(nb_page), int(nb_pos)
        self.n_pages, self.pages, self.d_len, self.n_kv_max = int(n_pages), pages, d_len, int(n_kv_max)

    @property
    def n_seq(self):
        return self.pages.shape[0]


def kv_store_latent_paged(lc, x):
    """x f32 [n_seq * n_q, 576] (last stride 1) -> row (b, t) to its page row at position d_len[b] + t, bit for bit kv_store's bytes at row_elems = 576; a
    position outside [0, n_kv_max) or a page id outside [0, n_pages) writes nothing.  The rotation of columns 512 .. 575 is the caller's: rope() in place on
    x[:, 512:].unsqueeze(1) first."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == MLA_DK
    assert x.shape[0] % lc.n_seq == 0, "n_seq * n_q rows"
    check(lib().ggml_hip_kv_store_latent_paged_dev(lc.kv_type, C.c_void_p(x.data_ptr()), x.stride(0), lc.n_seq, x.shape[0] // lc.n_seq,
                                                   C.c_void_p(lc.pool.data_ptr()), lc.nb_page, lc.nb_pos, lc.n_pages, C.c_void_p(lc.pages.data_ptr()),
                                                   lc.pages.stride(0), C.c_void_p(lc.d_len.data_ptr()), lc.n_kv_max, _stream()), "ggml_hip_kv_store_latent_paged_dev")


def attn_mla_paged(lc, q, scale, len_bias=0, causal=True, out=None, work=None):
    """attention_mla of n_seq independent sequences over the paged latent cache lc in one call: q f32 [n_seq * n_q, n_head, 576], sequence b over its
    n_kv[b] = clamp(d_len[b] + len_bias, 0, n_kv_max) positions; its rows are bit for bit attention_mla() on a contiguous copy of its cache.  A sequence
    with n_kv 0 or an invalid needed page id returns +0.0 rows."""
    assert q.is_cuda and q.dtype == torch.float32 and q.dim() == 3 and q.stride(2) == 1 and q.shape[2] == MLA_DK
    n_rows, n_head, _ = q.shape
    assert n_rows % lc.n_seq == 0, "n_seq * n_q rows"
    n_q = n_rows // lc.n_seq
    if out is None:
        out = torch.empty((n_rows, n_head, MLA_DV), dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and out.dim() == 3 and out.stride(2) == 1 and tuple(out.shape) == (n_rows, n_head, MLA_DV)
    if work is None:
        work = torch.empty(max(attn_mla_work_size(lc.kv_type, n_head, n_q, lc.n_kv_max, lc.n_seq), 16), dtype=torch.uint8, device=q.device)
    check(lib().ggml_hip_attn_mla_paged_dev(lc.kv_type, C.c_void_p(q.data_ptr()), q.stride(0), q.stride(1), C.c_void_p(lc.pool.data_ptr()), lc.nb_page, lc.nb_pos,
                                            lc.n_pages, C.c_void_p(lc.pages.data_ptr()), lc.pages.stride(0), C.c_void_p(lc.d_len.data_ptr()), int(len_bias),
                                            lc.n_seq, n_head, MLA_DK, MLA_DV, n_q, lc.n_kv_max, int(bool(causal)), float(scale), C.c_void_p(out.data_ptr()),
                                            out.stride(0), out.stride(1), C.c_void_p(work.data_ptr()), work.numel(), _stream()), "ggml_hip_attn_mla_paged_dev")
    return out


def _ragged(pc, q_start, x):
    """(n_tokens_max, heads, D) of packed rows x [n_tokens_max, heads, D] under q_start int32 [n_seq + 1] on the device"""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.stride(2) == 1
    assert q_start.is_cuda and q_start.dtype == torch.int32 and q_start.is_contiguous() and q_start.numel() == pc.n_seq + 1
    return x.shape


def ragged_positions(q_start, d_len, n_tokens_max, out=None):
    """out[i] = d_len[b] + t for packed row i = (b, t) of a present sequence (0 <= q_start[b] <= q_start[b+1] <= n_tokens_max), 0 for the other rows:
    the int32 position tensor rope() takes for Q, computed on the device so that a captured step follows q_start"""
    assert q_start.is_cuda and q_start.dtype == torch.int32 and q_start.is_contiguous()
    assert d_len.is_cuda and d_len.dtype == torch.int32 and d_len.is_contiguous() and d_len.numel() + 1 == q_start.numel()
    if out is None:
        out = torch.empty((n_tokens_max,), dtype=torch.int32, device=q_start.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == n_tokens_max
    check(lib().ggml_hip_ragged_positions_dev(C.c_void_p(q_start.data_ptr()), C.c_void_p(d_len.data_ptr()), d_len.numel(), n_tokens_max,
                                              C.c_void_p(out.data_ptr()), _stream()), "ggml_hip_ragged_positions_dev")
    return out


def kv_store_paged_ragged(pc, q_start, x, pool):
    """kv_store_paged over packed rows: x f32 [n_tokens_max, n_head_kv, D], the rows of sequence b at q_start[b] .. q_start[b+1] - 1 (q_start int32
    [n_seq + 1] on the device); the same bytes per row, nothing for a row of no present sequence"""
    n_tokens_max, n_head_kv, D = _ragged(pc, q_start, x)
    nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len = pc._args()
    check(lib().ggml_hip_kv_store_paged_ragged_dev(pc.kv_type, C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), n_head_kv, D, pc.n_seq,
                                                   C.c_void_p(q_start.data_ptr()), n_tokens_max, C.c_void_p(pool.data_ptr()), nbp, nbo, nbh, n_pages, d_pages,
                                                   ld_pages, d_len, pc.n_kv_max, _stream()), "ggml_hip_kv_store_paged_ragged_dev")


def rope_kv_store_paged_ragged(rp, pc, q_start, x, pool, freq_factors=None):
    """rope_kv_store_paged over packed rows (see kv_store_paged_ragged): the same bytes per row"""
    assert freq_factors is None or (freq_factors.is_cuda and freq_factors.dtype == torch.float32 and freq_factors.is_contiguous())
    n_tokens_max, n_head_kv, D = _ragged(pc, q_start, x)
    nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len = pc._args()
    check(lib().ggml_hip_rope_kv_store_paged_ragged_dev(C.byref(rp), pc.kv_type, C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), n_head_kv, D, pc.n_seq,
                                                        C.c_void_p(q_start.data_ptr()), n_tokens_max, _opt(freq_factors), C.c_void_p(pool.data_ptr()), nbp, nbo,
                                                        nbh, n_pages, d_pages, ld_pages, d_len, pc.n_kv_max, _stream()), "ggml_hip_rope_kv_store_paged_ragged_dev")


def attn_paged_ragged_plan(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max, window=0, softcap=0.0):
    """the ggml_hip_attn_ragged_plan_t of one ragged call: four launches sized by the bounds alone; no device needed"""
    out = _lib.ggml_hip_attn_ragged_plan_t()
    opts = _lib.ggml_hip_attn_opts_t(None, int(window), float(softcap), 0)
    check(lib().ggml_hip_attn_paged_ragged_plan(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max, C.byref(opts), C.byref(out)),
          "ggml_hip_attn_paged_ragged_plan")
    return out


def attn_paged_ragged_work_size(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max):
    return int(lib().ggml_hip_attn_paged_ragged_work_size(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max))


def attn_paged_ragged(pc, q_start, q, n_head_kv, add_q=False, len_bias=0, n_dec_rows_max=None, causal=True, scale=None, out=None, work=None, window=0,
                      softcap=0.0, sinks=None, mask=None, slopes=None):
    """attn_paged with a query count per sequence read on the device: q f32 [n_tokens_max, n_head, D] packed, the rows of sequence b at q_start[b] ..
    q_start[b+1] - 1 (q_start int32 [n_seq + 1] on the device), over n_kv[b] = clamp(d_len[b] + (add_q ? n_q[b] : 0) + len_bias, 0, n_kv_max) positions.
    A sequence's rows are bit for bit attn_paged for it alone; the form (DECODE up to 8 rows, PROMPT above) follows n_q[b] per sequence.
    n_dec_rows_max (default min(n_tokens_max, 8 n_seq), which never overflows) bounds the DECODE rows of the work buffer: a DECODE sequence that does
    not fit returns +0.0 rows.  out must be given for rows of no present sequence to keep what they held: they are not written.
    mask (f16 [n_tokens_max, >= n_kv_max], row = the packed row, column = the position in that row's own sequence) and slopes: as attention(), through
    ggml_hip_attn_paged_ragged_bias_dev."""
    assert q_start.is_cuda and q_start.dtype == torch.int32 and q_start.is_contiguous() and q_start.numel() == pc.n_seq + 1
    assert q.is_cuda and q.dtype == torch.float32 and q.dim() == 3 and q.stride(2) == 1
    n_tokens_max, n_head, D = q.shape
    if n_dec_rows_max is None:
        n_dec_rows_max = min(n_tokens_max, 8 * pc.n_seq)
    if scale is None:
        scale = 1.0 / float(np.sqrt(np.float64(D)))
    if out is None:
        out = torch.zeros((n_tokens_max, n_head, D), dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and out.dim() == 3 and out.stride(2) == 1 and tuple(out.shape) == (n_tokens_max, n_head, D)
    if work is None:
        work = torch.empty(max(attn_paged_ragged_work_size(pc.kv_type, D, n_head, n_head_kv, pc.n_seq, n_tokens_max, n_dec_rows_max, pc.n_kv_max), 16),
                           dtype=torch.uint8, device=q.device)
    nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len = pc._args()
    opts = attn_opts(window, softcap, sinks)
    bias = attn_bias(mask, slopes)
    if bias is not None:
        check(lib().ggml_hip_attn_paged_ragged_bias_dev(pc.kv_type, C.c_void_p(q.data_ptr()), q.stride(0), q.stride(1), C.c_void_p(pc.k.data_ptr()),
                                                        C.c_void_p(pc.v.data_ptr()), nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len, int(bool(add_q)),
                                                        int(len_bias), pc.n_seq, C.c_void_p(q_start.data_ptr()), n_tokens_max, int(n_dec_rows_max), n_head,
                                                        n_head_kv, D, pc.n_kv_max, int(bool(causal)), float(scale),
                                                        C.byref(opts) if opts is not None else None, C.byref(bias), C.c_void_p(out.data_ptr()),
                                                        out.stride(0), out.stride(1), C.c_void_p(work.data_ptr()), work.numel(), _stream()),
              "ggml_hip_attn_paged_ragged_bias_dev")
        return out
    check(lib().ggml_hip_attn_paged_ragged_dev(pc.kv_type, C.c_void_p(q.data_ptr()), q.stride(0), q.stride(1), C.c_void_p(pc.k.data_ptr()),
                                               C.c_void_p(pc.v.data_ptr()), nbp, nbo, nbh, n_pages, d_pages, ld_pages, d_len, int(bool(add_q)), int(len_bias),
                                               pc.n_seq, C.c_void_p(q_start.data_ptr()), n_tokens_max, int(n_dec_rows_max), n_head, n_head_kv, D, pc.n_kv_max,
                                               int(bool(causal)), float(scale), C.byref(opts) if opts is not None else None, C.c_void_p(out.data_ptr()),
                                               out.stride(0), out.stride(1), C.c_void_p(work.data_ptr()), work.numel(), _stream()),
          "ggml_hip_attn_paged_ragged_dev")
    return out


def get_rows(w, ids, out=None):
    """out[i, :K] = dequantize(w[ids[i]]) on the current stream: ids an int32 tensor on the device; bit for bit download + dequantize, a row of
    +0.0 for an id outside [0, M).  out f32 [n_ids, >= K] with last stride 1 (default a new [n_ids, K] tensor)."""
    assert ids.is_cuda and ids.dtype == torch.int32 and ids.is_contiguous()
    n = ids.numel()
    if out is None:
        out = torch.empty((n, w.K), dtype=torch.float32, device=ids.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= n
    check(lib().ggml_hip_get_rows_dev(w.handle, C.c_void_p(ids.data_ptr()), n, C.c_void_p(out.data_ptr()), out.stride(0), _stream()), "ggml_hip_get_rows_dev")
    return out


def topk_work(n_rows, n_vocab, k, device=None):
    """the work buffer ggml_hip_argmax_rows_dev (k = 1) / ggml_hip_sample_topk_dev need for a shape"""
    return torch.empty(max(int(lib().ggml_hip_topk_work_size(n_rows, n_vocab, k)), 8), dtype=torch.uint8, device=device or "cuda")


def argmax_rows(logits, ids=None, work=None):
    """ids[r] = the index of the largest logit of row r (ties: the smaller index; a NaN below every number): logits f32 [n_rows, n_vocab], last
    stride 1.  ids: an int32 tensor on the device (default new) -- the one get_rows() reads on the next step."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    n_rows, n_vocab = logits.shape
    if ids is None:
        ids = torch.empty(n_rows, dtype=torch.int32, device=logits.device)
    if work is None:
        work = topk_work(n_rows, n_vocab, 1, logits.device)
    assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.numel() >= n_rows
    check(lib().ggml_hip_argmax_rows_dev(C.c_void_p(logits.data_ptr()), logits.stride(0), n_rows, n_vocab, C.c_void_p(ids.data_ptr()), C.c_void_p(work.data_ptr()),
                                         work.numel(), _stream()), "ggml_hip_argmax_rows_dev")
    return ids


def sample_topk(logits, k, inv_temp=1.0, top_p=1.0, u=None, ids=None, probs=None, token=None, work=None, want_probs=True):
    """the k best logits of every row (ids [n_rows, k], rank order), p = softmax((l - l_0) * inv_temp) over them (probs [n_rows, k]) and, with
    u (f32 [n_rows] uniforms in [0, 1) on the device), the pick among the top_p mass (token int32 [n_rows]).  -> (ids, probs, token); probs is
    None with want_probs = False (then no pick), token is None without u."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    n_rows, n_vocab = logits.shape
    dev = logits.device
    if ids is None:
        ids = torch.empty((n_rows, k), dtype=torch.int32, device=dev)
    if probs is None and want_probs:
        probs = torch.empty((n_rows, k), dtype=torch.float32, device=dev)
    if u is not None and token is None:
        token = torch.empty(n_rows, dtype=torch.int32, device=dev)
    if work is None:
        work = topk_work(n_rows, n_vocab, k, dev)
    assert ids.dtype == torch.int32 and ids.is_contiguous() and (probs is None or (probs.dtype == torch.float32 and probs.is_contiguous()))
    assert u is None or (u.is_cuda and u.dtype == torch.float32 and u.is_contiguous() and token.dtype == torch.int32)
    check(lib().ggml_hip_sample_topk_dev(C.c_void_p(logits.data_ptr()), logits.stride(0), n_rows, n_vocab, int(k), float(inv_temp), float(top_p), _opt(u),
                                         C.c_void_p(ids.data_ptr()), _opt(probs), _opt(token if u is not None else None), C.c_void_p(work.data_ptr()),
                                         work.numel(), _stream()), "ggml_hip_sample_topk_dev")
    return ids, probs, (token if u is not None else None)


def ragged_last_rows(x, q_start, n_tokens_max=None, out=None):
    """out[s] = x[q_start[s + 1] - 1] for every sequence s of a ragged step that is present and not empty, a row of +0.0 otherwise: the rows the LM head needs,
    gathered on the device so that a captured step follows q_start.  x f32 [n_tokens_max, K] with last stride 1, q_start int32 [n_seq + 1] on the device."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    assert q_start.is_cuda and q_start.dtype == torch.int32 and q_start.is_contiguous() and q_start.numel() >= 2
    n_seq, K = q_start.numel() - 1, x.shape[1]
    if n_tokens_max is None:
        n_tokens_max = x.shape[0]
    assert n_tokens_max <= x.shape[0]
    if out is None:
        out = torch.empty((n_seq, K), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= n_seq and out.shape[1] >= K
    check(lib().ggml_hip_ragged_last_rows_dev(C.c_void_p(x.data_ptr()), x.stride(0), C.c_void_p(q_start.data_ptr()), n_seq, n_tokens_max, K,
                                              C.c_void_p(out.data_ptr()), out.stride(0), _stream()), "ggml_hip_ragged_last_rows_dev")
    return out


def ssm_scan_plan(n_head, head_dim, d_state, n_group=1, n_seq=1):
    """the ggml_hip_ssm_plan_t of one selective-scan call: the form, the lanes of a state row, the workgroups; no device needed"""
    out = _lib.ggml_hip_ssm_plan_t()
    check(lib().ggml_hip_ssm_scan_plan(n_head, head_dim, d_state, n_group, n_seq, C.byref(out)), "ggml_hip_ssm_scan_plan")
    return out


def ssm_state_bytes(n_head, head_dim, d_state):
    return int(lib().ggml_hip_ssm_state_bytes(n_head, head_dim, d_state))


def ssm_conv_state_bytes(n_ch, d_conv):
    return int(lib().ggml_hip_ssm_conv_state_bytes(n_ch, d_conv))


def _ssm_batch(q_start, d_len, slot, state):
    """(n_seq, nb_slot, n_slots) of a ragged SSM batch: q_start int32 [n_seq + 1], d_len / slot int32 [n_seq], state f32 [n_slots, >= slot elements]"""
    assert q_start.is_cuda and q_start.dtype == torch.int32 and q_start.is_contiguous() and q_start.numel() >= 2
    n_seq = q_start.numel() - 1
    for t in (d_len, slot):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n_seq
    assert state.is_cuda and state.dtype == torch.float32 and state.dim() == 2 and state.stride(1) == 1
    return n_seq, state.stride(0) * 4, state.shape[0]


def ssm_conv_ragged(x, w, q_start, d_len, slot, state, bias=None, act=False, n_tokens_max=None, out=None):
    """upstream's ggml_ssm_conv over a ragged batch: x f32 [n_tokens_max, n_ch] packed rows (last stride 1), w f32 [n_ch, d_conv], bias f32 [n_ch] or
    None, act: a plain f32 silu behind it.  Sequence b owns rows q_start[b] .. q_start[b+1] - 1 and the slot state[slot[b]] ([d_conv - 1, n_ch] f32): the
    window starts from zeros where d_len[b] == 0 (the slot is not read), from the slot otherwise, and the slot then holds the sequence's last d_conv - 1
    rows.  A slot id outside the pool gives +0.0 rows and writes no state.  out may be x.  Rows of no present sequence are not written."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    assert w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and w.shape[0] == x.shape[1]
    assert bias is None or (bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == x.shape[1])
    n_seq, nb_slot, n_slots = _ssm_batch(q_start, d_len, slot, state)
    n_ch, d_conv = w.shape
    if n_tokens_max is None:
        n_tokens_max = x.shape[0]
    assert n_tokens_max <= x.shape[0]
    if out is None:
        out = torch.zeros((x.shape[0], n_ch), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= n_tokens_max and out.shape[1] >= n_ch
    check(lib().ggml_hip_ssm_conv_ragged_dev(C.c_void_p(x.data_ptr()), x.stride(0), C.c_void_p(w.data_ptr()), _opt(bias), int(bool(act)), n_ch, d_conv, n_seq,
                                             C.c_void_p(q_start.data_ptr()), n_tokens_max, C.c_void_p(d_len.data_ptr()), C.c_void_p(slot.data_ptr()),
                                             C.c_void_p(state.data_ptr()), nb_slot, n_slots, C.c_void_p(out.data_ptr()), out.stride(0), _stream()),
          "ggml_hip_ssm_conv_ragged_dev")
    return out


def ssm_conv_tiled_plan(n_ch, d_conv, n_seq=1, n_tokens_max=0):
    """the ggml_hip_ssm_conv_plan_t of one tiled-conv call: the form, the tile T, seq_max_tokens, the bounds of the tile list, the work bytes; no device
    needed"""
    out = _lib.ggml_hip_ssm_conv_plan_t()
    check(lib().ggml_hip_ssm_conv_tiled_plan(n_ch, d_conv, n_seq, n_tokens_max, C.byref(out)), "ggml_hip_ssm_conv_tiled_plan")
    return out


def ssm_conv_tiled_work_size(n_ch, d_conv, n_seq=1, n_tokens_max=0):
    return int(lib().ggml_hip_ssm_conv_tiled_work_size(n_ch, d_conv, n_seq, n_tokens_max))


def ssm_conv_tiled_ragged(x, w, q_start, d_len, slot, state, bias=None, act=False, n_tokens_max=None, out=None, work=None):
    """ssm_conv_ragged with the token-parallel tiled form for the sequences of more than seq_max_tokens tokens in this call (ssm_conv_tiled_plan): the
    same bits in both forms, wherever a sequence is split over calls.  work: a uint8 tensor of at least ssm_conv_tiled_work_size(..) bytes (a captured
    step passes its own); None allocates one.  out may be x."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    assert w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and w.shape[0] == x.shape[1]
    assert bias is None or (bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == x.shape[1])
    n_seq, nb_slot, n_slots = _ssm_batch(q_start, d_len, slot, state)
    n_ch, d_conv = w.shape
    if n_tokens_max is None:
        n_tokens_max = x.shape[0]
    assert n_tokens_max <= x.shape[0]
    if out is None:
        out = torch.zeros((x.shape[0], n_ch), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= n_tokens_max and out.shape[1] >= n_ch
    need = ssm_conv_tiled_work_size(n_ch, d_conv, n_seq, n_tokens_max)
    if work is None and need:
        work = torch.empty(need, dtype=torch.uint8, device=x.device)
    assert work is None or (work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous() and work.numel() >= need)
    check(lib().ggml_hip_ssm_conv_tiled_ragged_dev(C.c_void_p(x.data_ptr()), x.stride(0), C.c_void_p(w.data_ptr()), _opt(bias), int(bool(act)), n_ch, d_conv,
                                                   n_seq, C.c_void_p(q_start.data_ptr()), n_tokens_max, C.c_void_p(d_len.data_ptr()),
                                                   C.c_void_p(slot.data_ptr()), C.c_void_p(state.data_ptr()), nb_slot, n_slots, C.c_void_p(out.data_ptr()),
                                                   out.stride(0), _opt(work), 0 if work is None else work.numel(), _stream()),
          "ggml_hip_ssm_conv_tiled_ragged_dev")
    return out


def ssm_scan_ragged(x, dt, A, B, C_, q_start, d_len, slot, state, dt_bias=None, D=None, n_tokens_max=None, out=None):
    """upstream's ggml_ssm_scan over a ragged batch: x f32 [n_tokens_max, n_head, P] (last stride 1), dt f32 [n_tokens_max, n_head], A f32 [n_head]
    (one value per head, Mamba-2) or [n_head, N] (per state, Mamba-1), B / C_ f32 [n_tokens_max, G, N] views with ONE token stride and contiguous groups,
    dt_bias / D f32 [n_head] or None.  Per token: delta = softplus(dt + dt_bias), h = h * exp(delta * A) + (delta * x) * B, y = sum_n h_n C_n + D x, in
    the order include/ggml_hip_ext.h fixes.  Sequence b continues from state[slot[b]] ([n_head, P, N] f32; zeros where d_len[b] == 0, the slot is not
    read) and leaves its final state there.  A sequence's bits do not depend on the batch or on how its tokens are split over calls."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.stride(2) == 1
    n_rows, n_head, P = x.shape
    assert dt.is_cuda and dt.dtype == torch.float32 and dt.dim() == 2 and dt.stride(1) == 1 and dt.shape[1] == n_head
    assert A.is_cuda and A.dtype == torch.float32 and A.dim() in (1, 2) and A.shape[0] == n_head and A.stride(-1) == 1
    for t in (B, C_):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2]
    assert B.shape == C_.shape and B.stride(0) == C_.stride(0)
    G, N = B.shape[1], B.shape[2]
    for t in (dt_bias, D):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n_head)
    n_seq, nb_slot, n_slots = _ssm_batch(q_start, d_len, slot, state)
    if n_tokens_max is None:
        n_tokens_max = n_rows
    assert n_tokens_max <= min(n_rows, dt.shape[0], B.shape[0])
    if out is None:
        out = torch.zeros((n_rows, n_head, P), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 3 and out.stride(2) == 1 and tuple(out.shape) == (n_rows, n_head, P)
    per_state = A.dim() == 2
    check(lib().ggml_hip_ssm_scan_ragged_dev(C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), C.c_void_p(dt.data_ptr()), dt.stride(0), _opt(dt_bias),
                                             C.c_void_p(A.data_ptr()), A.stride(0), int(per_state), C.c_void_p(B.data_ptr()), C.c_void_p(C_.data_ptr()),
                                             B.stride(0), _opt(D), n_head, P, N, G, n_seq, C.c_void_p(q_start.data_ptr()), n_tokens_max,
                                             C.c_void_p(d_len.data_ptr()), C.c_void_p(slot.data_ptr()), C.c_void_p(state.data_ptr()), nb_slot, n_slots,
                                             C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1), _stream()), "ggml_hip_ssm_scan_ragged_dev")
    return out


def ssm_scan_chunked_plan(n_head, head_dim, d_state, n_group=1, a_per_state=False, n_seq=1, n_tokens_max=0):
    """the ggml_hip_ssm_chunk_plan_t of one chunked-scan call: the form, the chunk Q, seq_max_tokens, the bounds of the chunk list, the work bytes; no
    device needed"""
    out = _lib.ggml_hip_ssm_chunk_plan_t()
    check(lib().ggml_hip_ssm_scan_chunked_plan(n_head, head_dim, d_state, n_group, int(bool(a_per_state)), n_seq, n_tokens_max, C.byref(out)),
          "ggml_hip_ssm_scan_chunked_plan")
    return out


def ssm_scan_chunked_work_size(n_head, head_dim, d_state, n_group=1, a_per_state=False, n_seq=1, n_tokens_max=0):
    return int(lib().ggml_hip_ssm_scan_chunked_work_size(n_head, head_dim, d_state, n_group, int(bool(a_per_state)), n_seq, n_tokens_max))


def ssm_scan_chunked_ragged(x, dt, A, B, C_, q_start, d_len, slot, state, dt_bias=None, D=None, n_tokens_max=None, out=None, work=None):
    """ssm_scan_ragged with the chunked matrix form for the sequences of more than seq_max_tokens tokens in this call (ssm_scan_chunked_plan); the shorter
    ones are bit for bit ssm_scan_ragged's.  work: a uint8 tensor of at least ssm_scan_chunked_work_size(..) bytes (a captured step passes its own);
    None allocates one.  Splitting a long sequence over calls keeps its bits only at multiples of the chunk."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.stride(2) == 1
    n_rows, n_head, P = x.shape
    assert dt.is_cuda and dt.dtype == torch.float32 and dt.dim() == 2 and dt.stride(1) == 1 and dt.shape[1] == n_head
    assert A.is_cuda and A.dtype == torch.float32 and A.dim() in (1, 2) and A.shape[0] == n_head and A.stride(-1) == 1
    for t in (B, C_):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2]
    assert B.shape == C_.shape and B.stride(0) == C_.stride(0)
    G, N = B.shape[1], B.shape[2]
    for t in (dt_bias, D):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n_head)
    n_seq, nb_slot, n_slots = _ssm_batch(q_start, d_len, slot, state)
    if n_tokens_max is None:
        n_tokens_max = n_rows
    assert n_tokens_max <= min(n_rows, dt.shape[0], B.shape[0])
    if out is None:
        out = torch.zeros((n_rows, n_head, P), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 3 and out.stride(2) == 1 and tuple(out.shape) == (n_rows, n_head, P)
    per_state = A.dim() == 2
    need = ssm_scan_chunked_work_size(n_head, P, N, G, per_state, n_seq, n_tokens_max)
    if work is None and need:
        work = torch.empty(need, dtype=torch.uint8, device=x.device)
    assert work is None or (work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous() and work.numel() >= need)
    check(lib().ggml_hip_ssm_scan_chunked_ragged_dev(C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), C.c_void_p(dt.data_ptr()), dt.stride(0), _opt(dt_bias),
                                                     C.c_void_p(A.data_ptr()), A.stride(0), int(per_state), C.c_void_p(B.data_ptr()), C.c_void_p(C_.data_ptr()),
                                                     B.stride(0), _opt(D), n_head, P, N, G, n_seq, C.c_void_p(q_start.data_ptr()), n_tokens_max,
                                                     C.c_void_p(d_len.data_ptr()), C.c_void_p(slot.data_ptr()), C.c_void_p(state.data_ptr()), nb_slot, n_slots,
                                                     C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1), _opt(work), 0 if work is None else work.numel(),
                                                     _stream()), "ggml_hip_ssm_scan_chunked_ragged_dev")
    return out


def quantize_rows(type, x):
    """x f32 [nrows, k] on the device -> uint8 [nrows, k/32*type_size] reference-format blocks."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    nrows, k = x.shape
    out = torch.empty((nrows, row_bytes(type, k)), dtype=torch.uint8, device=x.device)
    check(lib().ggml_hip_quantize_rows_dev(type, C.c_void_p(x.data_ptr()), nrows, k, C.c_void_p(out.data_ptr()),
                                           _stream()), "ggml_hip_quantize_rows_dev")
    return out


def quantize_rows_from(type, x):
    """x f32 or f16 [nrows, k] on the device (row stride may exceed k) -> reference-format blocks."""
    assert x.is_cuda and x.dim() == 2 and x.stride(1) == 1 and x.dtype in (torch.float32, torch.float16)
    nrows, k = x.shape
    out = torch.empty((nrows, row_bytes(type, k)), dtype=torch.uint8, device=x.device)
    check(lib().ggml_hip_quantize_rows_src_dev(type, 0 if x.dtype == torch.float32 else 1, C.c_void_p(x.data_ptr()),
                                               x.stride(0), nrows, k, C.c_void_p(out.data_ptr()), _stream()),
          "ggml_hip_quantize_rows_src_dev")
    return out


def add_q_f32_rows(type, blocks, x):
    """blocks uint8 [nrows, k/32*type_size], x f32 [nrows, k] -> quantize(dequantize(blocks) + x)."""
    assert blocks.is_cuda and x.is_cuda and blocks.is_contiguous() and x.is_contiguous() and x.dtype == torch.float32
    nrows, k = x.shape
    out = torch.empty_like(blocks)
    check(lib().ggml_hip_add_q_f32_rows_dev(type, C.c_void_p(blocks.data_ptr()), C.c_void_p(x.data_ptr()), nrows, k,
                                            C.c_void_p(out.data_ptr()), _stream()), "ggml_hip_add_q_f32_rows_dev")
    return out


def dequantize_rows(type, blocks, k):
    assert blocks.is_cuda and blocks.dtype == torch.uint8 and blocks.is_contiguous()
    nrows = blocks.numel() // row_bytes(type, k)
    out = torch.empty((nrows, k), dtype=torch.float32, device=blocks.device)
    check(lib().ggml_hip_dequantize_rows_dev(type, C.c_void_p(blocks.data_ptr()), nrows, k,
                                             C.c_void_p(out.data_ptr()), _stream()), "ggml_hip_dequantize_rows_dev")
    return out


def relayout_gathered(gathered, G, N, Ms, M, out=None):
    if out is None:
        out = torch.empty((N, M), dtype=torch.float32, device=gathered.device)
    check(lib().ggml_hip_relayout_gathered_dev(C.c_void_p(gathered.data_ptr()), G, N, Ms, C.c_void_p(out.data_ptr()),
                                               M, out.stride(0), _stream()), "ggml_hip_relayout_gathered_dev")
    return out
