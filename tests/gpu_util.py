"""Thin helpers for the `-m gpu` parity tests: frame-row buffers (csrc/common.h layout) and ctypes calls
through the C ABI single-op entry points."""
import ctypes as C

import torch

from wfl_asr_amd import _lib


def lib():
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, elem_off=0):
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr() + elem_off * t.element_size())


class Rows:
    """bf16 frame rows: row(b, t) = lead + b*P + t, zero halos."""

    def __init__(self, B, T, C_, halo=16, lead=16, tail=256, pitch=None, device="cuda"):
        self.B, self.T, self.C = B, T, C_
        self.P = pitch if pitch is not None else (T + halo + 7) // 8 * 8
        self.lead, self.tail = lead, tail
        self.R = lead + B * self.P + tail
        self.buf = torch.zeros(self.R, C_, dtype=torch.bfloat16, device=device)

    def set(self, x):                      # x [B, T, C] float
        v = self.buf[self.lead:self.lead + self.B * self.P].view(self.B, self.P, self.C)
        v[:, :self.T] = x.to(torch.bfloat16)
        return self

    def get(self):                         # -> [B, T, C] float32
        v = self.buf[self.lead:self.lead + self.B * self.P].view(self.B, self.P, self.C)
        return v[:, :self.T].float()

    def halo_is_zero(self):
        v = self.buf[self.lead:self.lead + self.B * self.P].view(self.B, self.P, self.C)
        return bool((v[:, self.T:] == 0).all() and (self.buf[:self.lead] == 0).all()
                    and (self.buf[self.lead + self.B * self.P:] == 0).all())


def pad_weight(w, bias=None):
    """[N, K] float -> bf16 [N128, K64] + fp32 bias [N128]."""
    N, K = w.shape
    Np, Kp = (N + 127) // 128 * 128, (K + 63) // 64 * 64
    wp = torch.zeros(Np, Kp, dtype=torch.bfloat16, device=w.device)
    wp[:N, :K] = w.to(torch.bfloat16)
    bp = torch.zeros(Np, dtype=torch.float32, device=w.device)
    if bias is not None:
        bp[:N] = bias
    return wp, bp


def gemm(A, a_off, lda, Wp, M, n_valid, P, T, Cout, c_ld, c_lead, c_pitch, bias=None, res=None, ldres=0, alpha=1.0,
         act=0, glu=0, out_f32=0, cin=0, tap_stride=0):
    N, K = Wp.shape
    rc = lib().wfl_op_gemm(ptr(A, a_off), lda, cin, tap_stride, ptr(Wp), M, N, K, n_valid, P, T, ptr(Cout), c_ld, c_lead,
                           c_pitch, ptr(bias), ptr(res), ldres, float(alpha), act, glu, out_f32, stream())
    _lib.check(rc, "wfl_op_gemm")


def gemm_ln(A, a_off, lda, Wp, M, n_valid, P, T, Cout, c_ld, c_lead, c_pitch, bias, ln_s, eps=1e-5, act=0):
    N, K = Wp.shape
    rc = lib().wfl_op_gemm_ln(ptr(A, a_off), lda, ptr(Wp), M, N, K, n_valid, P, T, ptr(Cout), c_ld, c_lead, c_pitch, ptr(bias),
                              ptr(ln_s), float(eps), act, stream())
    _lib.check(rc, "wfl_op_gemm_ln")


_GEMM_EX_POINTERS = {n for n, t in _lib.WflGemmExArgs._fields_ if t is C.c_void_p}


def gemm_ex(check=True, **fields):
    """wfl_op_gemm_ex: the fields of include/wfl_asr.h's wfl_gemm_ex_args by name.  Pointer fields take a device tensor, a
    (tensor, element offset) pair or None; everything else a number.  -> (status code, kernel id)."""
    a = _lib.WflGemmExArgs()
    for k, v in fields.items():
        if k in _GEMM_EX_POINTERS:
            v = ptr(*v) if isinstance(v, tuple) else ptr(v)
        elif k not in {n for n, _ in _lib.WflGemmExArgs._fields_}:
            raise TypeError(f"wfl_gemm_ex_args has no field {k}")
        setattr(a, k, v)
    kid = C.c_int32(-1)
    rc = lib().wfl_op_gemm_ex(C.byref(a), C.byref(kid), stream())
    if check:
        _lib.check(rc, "wfl_op_gemm_ex")
    return rc, kid.value


def attention(QK, ldqk, lead, V, v_off, ldv, O, ldo, B, T, P, heads, d):
    _lib.check(lib().wfl_op_attention(ptr(QK), ldqk, lead, ptr(V, v_off), ldv, ptr(O), ldo, B, T, P, heads, d, stream()), "wfl_op_attention")


def layernorm(x, y, g, b, eps, lead, B, P, T, Cn):
    _lib.check(lib().wfl_op_layernorm(ptr(x), Cn, ptr(y), Cn, ptr(g), ptr(b), float(eps), lead, B, P, T, Cn, stream()), "wfl_op_layernorm")


def tag_decide(logits, thr, o_id):
    rows, Cn = logits.shape
    ids = torch.empty(rows, dtype=torch.int32, device=logits.device)
    arg = torch.empty_like(ids)
    mp = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _lib.check(lib().wfl_op_tag_decide(ptr(logits), Cn, rows, Cn, float(thr), o_id, ptr(ids), ptr(arg), ptr(mp), stream()), "wfl_op_tag_decide")
    return ids, arg, mp


def _i32(v):
    """list of ints -> int32 device tensor (None stays None)."""
    return None if v is None else torch.tensor(list(v), dtype=torch.int32, device="cuda")


def attention_ex(QK, ldqk, lead, V, v_off, ldv, O, ldo, B, T, P, heads, d, QK_lo=None, V_lo=None, O_lo=None, bias=None, gate=None,
                 clip_T=None, O8=None, O8_lo=None, ldo8=0, o8_scale=1.0, status=None, check=True):
    """wfl_op_attention_ex; clip_T an int32 device tensor.  -> the status code (check: raise on an error status)."""
    rc = lib().wfl_op_attention_ex(ptr(QK), ptr(QK_lo), ldqk, lead, ptr(V, v_off), ptr(V_lo, v_off) if V_lo is not None else ptr(None), ldv,
                                   ptr(O), ptr(O_lo), ldo, B, T, P, heads, d, ptr(bias), ptr(gate), ptr(clip_T), ptr(O8), ptr(O8_lo), ldo8,
                                   float(o8_scale), ptr(status), stream())
    if check:
        _lib.check(rc, "wfl_op_attention_ex")
    return rc


def relpos_table(rel_emb, bucket_of_delta, max_t, heads, T, table, check=True):
    rc = lib().wfl_op_relpos_table(ptr(rel_emb), ptr(bucket_of_delta), max_t, heads, T, ptr(table), stream())
    if check:
        _lib.check(rc, "wfl_op_relpos_table")
    return rc


def relpos_gate(x, x_lo, ldx, lead, B, P, T, heads, hd, w8, b8, cst, gate):
    _lib.check(lib().wfl_op_relpos_gate(ptr(x), ptr(x_lo), ldx, lead, B, P, T, heads, hd, ptr(w8), ptr(b8), ptr(cst), ptr(gate), stream()),
               "wfl_op_relpos_gate")


def regroup(x, d, groups, cpg, R, lead, B, P, T, xg, clip_T=None):
    _lib.check(lib().wfl_op_regroup(ptr(x), d, groups, cpg, R, lead, B, P, T, ptr(clip_T), ptr(xg), stream()), "wfl_op_regroup")


def posconv(xg, R, lead, B, P, T, groups, cpg, taps, w, ldw, bias, res, res_lo, out, out_lo, ld, clip_T=None, check=True):
    rc = lib().wfl_op_posconv(ptr(xg), R, lead, B, P, T, groups, cpg, taps, ptr(w), ldw, ptr(bias), ptr(res), ptr(res_lo), ptr(out),
                              ptr(out_lo), ld, ptr(clip_T), stream())
    if check:
        _lib.check(rc, "wfl_op_posconv")
    return rc


def layernorm_act(x, x_lo, y, y_lo, g, b, eps, lead, B, P, T, Cn, n_div=0, gelu=0, clip_T=None):
    _lib.check(lib().wfl_op_layernorm_act(ptr(x), ptr(x_lo), Cn, ptr(y), ptr(y_lo), Cn, ptr(g), ptr(b), float(eps), lead, B, P, T, Cn, n_div,
                                          gelu, ptr(clip_T), stream()), "wfl_op_layernorm_act")


def layernorm_pair(x, x_lo, y1, y1_lo, y2, y2_lo, g1, b1, g2, b2, eps, lead, B, P, T, Cn, n_div=0, clip_T=None):
    _lib.check(lib().wfl_op_layernorm_pair(ptr(x), ptr(x_lo), ptr(y1), ptr(y1_lo), ptr(y2), ptr(y2_lo), Cn, ptr(g1), ptr(b1), ptr(g2), ptr(b2),
                                           float(eps), lead, B, P, T, Cn, n_div, ptr(clip_T), stream()), "wfl_op_layernorm_pair")


def wav_stats(wav, ldw, B, L, stats, lens=None, check=True):
    """wfl_op_wav_stats: wav fp32 [B][ldw], stats float64 [2 B], lens int32 device tensor or None.  -> the status code."""
    rc = lib().wfl_op_wav_stats(ptr(wav), ldw, ptr(lens), B, L, ptr(stats), stream())
    if check:
        _lib.check(rc, "wfl_op_wav_stats")
    return rc


def clip_frames(lens, B, L, kernel, stride, min_len, out, n=None, check=True):
    """wfl_op_clip_frames: lens / out int32 device tensors, kernel / stride host lists (n: the level count passed, default their length)."""
    k = (C.c_int32 * max(len(kernel), 1))(*kernel)
    s = (C.c_int32 * max(len(stride), 1))(*stride)
    rc = lib().wfl_op_clip_frames(ptr(lens), B, L, len(kernel) if n is None else n, C.cast(k, C.c_void_p), C.cast(s, C.c_void_p), min_len,
                                  ptr(out), stream())
    if check:
        _lib.check(rc, "wfl_op_clip_frames")
    return rc


def conv0_scratch_bytes(B, T0, Cn):
    return int(lib().wfl_op_conv0_scratch_bytes(B, T0, Cn))


def conv0(wav, ldw, B, L, w, gamma, beta, Cn, T0, out, lead, P, group_norm, lens=None, wstats=None, bias=None, out_lo=None, scratch=None,
          scratch_bytes=None, check=True):
    """wfl_op_conv0; scratch a uint8 device tensor (group mode) or None.  -> the status code."""
    nbytes = (scratch.numel() if scratch is not None else 0) if scratch_bytes is None else scratch_bytes
    rc = lib().wfl_op_conv0(ptr(wav), ldw, ptr(lens), B, L, ptr(wstats), ptr(w), ptr(bias), ptr(gamma), ptr(beta), Cn, T0, ptr(out), ptr(out_lo),
                            lead, P, int(group_norm), ptr(scratch), nbytes, stream())
    if check:
        _lib.check(rc, "wfl_op_conv0")
    return rc


def lstm_exchange_bytes(H, B):
    return int(lib().wfl_op_lstm_exchange_bytes(H, B))


def lstm_pack_whh(whh, H, U=0, lo=True):
    """wfl_op_lstm_pack_whh: weight_hh of both directions [2, 4H, H] fp32 (CPU) -> the packed bf16 (hi, lo or None) on the device."""
    w = whh.detach().float().contiguous().numpy()
    hi = torch.empty(2 * 4 * H * H, dtype=torch.int16)
    lo_t = torch.empty_like(hi) if lo else None
    rc = lib().wfl_op_lstm_pack_whh(_lib.host_ptr(w), H, U, C.c_void_p(hi.data_ptr()), C.c_void_p(lo_t.data_ptr()) if lo else None)
    _lib.check(rc, "wfl_op_lstm_pack_whh")
    return hi.view(torch.bfloat16).cuda(), (lo_t.view(torch.bfloat16).cuda() if lo else None)


def lstm(gx, ldgx, whh, out, ldo, lead, B, T, P, H, exchange, status, U=0, whh_lo=None, out_lo=None, clip_T=None, exchange_bytes=None, check=True):
    """wfl_op_lstm: gx fp32 / out bf16 frame rows, whh (+ whh_lo) from lstm_pack_whh, clip_T an int32 device tensor or None, exchange a
    uint8 device tensor, status an int32 device tensor of one element.  -> the status code."""
    nbytes = exchange.numel() * exchange.element_size() if exchange_bytes is None else exchange_bytes
    rc = lib().wfl_op_lstm(ptr(gx), ldgx, ptr(whh), ptr(whh_lo), ptr(out), ptr(out_lo), ldo, lead, B, T, P, H, U, ptr(clip_T), ptr(exchange),
                           nbytes, ptr(status), stream())
    if check:
        _lib.check(rc, "wfl_op_lstm")
    return rc
