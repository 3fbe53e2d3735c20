"""ctypes binding of libwfl_asr_hip.so (include/wfl_asr.h).  Fails loudly when the HIP library is missing:
there is no CPU or eager-PyTorch fallback for the model forward anywhere in this package."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
# WFL_LIB_PATH: an alternative build of the same library (A/B runs of compiler flags: tools/build_variant.sh); never a fallback
LIB_PATH = os.environ.get("WFL_LIB_PATH") or os.path.join(PKG, "libwfl_asr_hip.so")
ABI_VERSION = 2


class WflArch(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("encoder_type", C.c_int32), ("d_model", C.c_int32), ("enc_layers", C.c_int32),
        ("enc_heads", C.c_int32), ("enc_ffn", C.c_int32), ("n_mels", C.c_int32), ("max_positions", C.c_int32),
        ("num_classes", C.c_int32), ("o_id", C.c_int32), ("num_languages", C.c_int32), ("lang_emb_dim", C.c_int32),
        ("enable_bilstm", C.c_int32), ("bilstm_layers", C.c_int32), ("n_conformer", C.c_int32),
        ("conformer_heads", C.c_int32), ("conformer_ff_expansion", C.c_int32), ("conformer_kernel", C.c_int32),
        ("enable_dilated", C.c_int32), ("dilated_depth", C.c_int32), ("dilated_kernel", C.c_int32),
        ("wavlm_n_conv", C.c_int32), ("wavlm_conv_dim", C.c_int32 * 8), ("wavlm_conv_kernel", C.c_int32 * 8),
        ("wavlm_conv_stride", C.c_int32 * 8), ("wavlm_group_norm", C.c_int32), ("wavlm_conv_bias", C.c_int32),
        ("wavlm_stable_layer_norm", C.c_int32), ("wavlm_pos_conv_kernel", C.c_int32),
        ("wavlm_pos_conv_groups", C.c_int32), ("wavlm_num_buckets", C.c_int32), ("wavlm_max_distance", C.c_int32),
        ("wavlm_do_normalize", C.c_int32), ("fp8_weights", C.c_int32), ("mel_hop", C.c_int32), ("precision", C.c_int32), ("fp8_activations", C.c_int32),
        ("mel_sample_rate", C.c_int32), ("reserved", C.c_int32 * 5),
    ]


_P = C.c_void_p
_I = C.c_int32
_L = C.c_int64
_F = C.c_float


class WflGemmExArgs(C.Structure):
    """include/wfl_asr.h's wfl_gemm_ex_args, field for field (struct_bytes is filled in by the constructor)."""
    _fields_ = [
        ("struct_bytes", _L),
        ("A", _P), ("lda", _L), ("tap_stride", _L), ("cin", _I), ("a8", _I),
        ("W", _P), ("w8_scale", _P), ("a8_scale", _P), ("a8_lead", _L), ("a8_static", _F),
        ("M", _I), ("N", _I), ("K", _I), ("n_valid", _I), ("P", _I), ("T", _I), ("c_pitch", _I),
        ("C", _P), ("c_lo", _P), ("ldc", _L), ("c_lead", _L),
        ("bias", _P), ("clip_bias", _P), ("clip_idx", _P), ("clip_T", _P), ("clip_ld", _I), ("act", _I),
        ("res", _P), ("res_lo", _P), ("ldres", _L), ("alpha", _F), ("glu", _I), ("out_f32", _I), ("acc_f32", _I),
        ("pos", _P), ("ldpos", _L),
        ("ln_s", _P), ("ln_eps", _F), ("stats_nsl", _I), ("stats_out", _P), ("stats_in", _P), ("stats_lead", _L),
        ("c8", _P), ("ldc8", _L), ("c8_inv_scale", _F), ("reserved", _I),
        ("status", _P),
    ]

    def __init__(self, **kw):
        super().__init__(**kw)
        if "struct_bytes" not in kw:
            self.struct_bytes = C.sizeof(WflGemmExArgs)

# name -> (restype, argtypes); exactly the declarations of include/wfl_asr.h
SIGNATURES = {
    "wfl_last_error": (C.c_char_p, []),
    "wfl_abi_version": (_I, []),
    "wfl_create": (_I, [C.POINTER(WflArch), C.POINTER(_P)]),
    "wfl_destroy": (None, [_P]),
    "wfl_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(_L), _I]),
    "wfl_finalize": (_I, [_P]),
    "wfl_num_frames": (_I, [_P, _I]),
    "wfl_workspace_bytes": (_L, [_P, _I, _I]),
    "wfl_device": (_I, [_P]),
    "wfl_set_average_languages": (_I, [_P, _P, _I]),
    "wfl_forward": (_I, [_P, _P, _L, _P, _I, _I, _P, _I, _F, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wfl_encode": (_I, [_P, _P, _L, _P, _I, _I, _P, _L, _P, _P]),
    "wfl_head_workspace_bytes": (_L, [_P, _I, _I]),
    "wfl_head": (_I, [_P, _P, _I, _I, _P, _I, _F, _P, _L, _P, _P, _P, _P, _P, _P, _P]),
    "wfl_check": (_I, [_P, _P, _L, _I, _I, _P]),
    "wfl_logmel": (_I, [_P, _P, _L, _P, _I, _I, _P, _P, _L, _P]),
    "wfl_op_gemm": (_I, [_P, _L, _I, _L, _P, _I, _I, _I, _I, _I, _I, _P, _L, _L, _I, _P, _P, _L, _F, _I, _I, _I, _P]),
    "wfl_op_gemm_ex": (_I, [C.POINTER(WflGemmExArgs), C.POINTER(_I), _P]),
    "wfl_op_gemm_split": (_I, [_P, _P, _L, _I, _L, _P, _I, _I, _I, _I, _I, _I, _P, _P, _L, _L, _I, _P, _P, _P, _L, _F, _I, _I, _P]),
    "wfl_op_gemm_ln": (_I, [_P, _L, _P, _I, _I, _I, _I, _I, _I, _P, _L, _L, _I, _P, _P, _F, _I, _P]),
    "wfl_op_gemm_mx": (_I, [_P, _P, _L, _P, _P, _P, _F, _I, _I, _I, _I, _I, _P, _L, _L, _I, _P, _P, _P, _P, _F, _I, _P, _P, _L, _F, _P, _P]),
    "wfl_op_rows_fp8": (_I, [_P, _L, _P, _P, _P, _F, _L, _I, _I, _I, _I, _P, _P, _L, _P, _P]),
    "wfl_op_attention": (_I, [_P, _L, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _P]),
    "wfl_op_attention_ex": (_I, [_P, _P, _L, _L, _P, _P, _L, _P, _P, _L, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _L, _F, _P, _P]),
    "wfl_op_relpos_table": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "wfl_op_relpos_gate": (_I, [_P, _P, _L, _L, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "wfl_op_regroup": (_I, [_P, _I, _I, _I, _L, _L, _I, _I, _I, _P, _P, _P]),
    "wfl_op_wav_stats": (_I, [_P, _L, _P, _I, _I, _P, _P]),
    "wfl_op_clip_frames": (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _P]),
    "wfl_op_conv0_scratch_bytes": (_L, [_I, _I, _I]),
    "wfl_op_conv0": (_I, [_P, _L, _P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _L, _I, _I, _P, _L, _P]),
    "wfl_op_posconv": (_I, [_P, _L, _L, _I, _I, _I, _I, _I, _I, _P, _L, _P, _P, _P, _P, _P, _L, _P, _P]),
    "wfl_op_layernorm_act": (_I, [_P, _P, _L, _P, _P, _L, _P, _P, _F, _L, _I, _I, _I, _I, _I, _I, _P, _P]),
    "wfl_op_layernorm_pair": (_I, [_P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _F, _L, _I, _I, _I, _I, _I, _P, _P]),
    "wfl_op_layernorm": (_I, [_P, _L, _P, _L, _P, _P, _F, _L, _I, _I, _I, _I, _P]),
    "wfl_op_tag_decide": (_I, [_P, _L, _I, _I, _F, _I, _P, _P, _P, _P]),
    "wfl_op_lstm_exchange_bytes": (_L, [_I, _I]),
    "wfl_op_lstm_pack_whh": (_I, [_P, _I, _I, _P, _P]),
    "wfl_op_lstm": (_I, [_P, _L, _P, _P, _P, _P, _L, _L, _I, _I, _I, _I, _I, _P, _P, _L, _P, _P]),
    "wfl_host_median_filter": (_I, [_P, _I, _I, _P]),
    "wfl_host_decode_bio": (_I, [_P, _I, _P, _I, _P, _P, _I, C.c_double, _P, _P, _P, _I]),
    "wfl_host_merge_segments": (_I, [_P, _P, _P, _I, _I]),
    "wfl_host_format_lab": (_L, [_P, _P, _P, _I, _P, _I, _P, _L]),
    "wfl_host_load_wav": (_I, [C.c_char_p, _P, _L, _P, _P]),
    "wfl_host_load_wavs": (_I, [_P, _I, _P, _L, _L, _P, _P, _P, _I]),
    "wfl_host_load_wav_chunks": (_I, [C.c_char_p, _I, _L, _P, _L, _I, _P, _P, _P]),
    "wfl_host_read_pcm16": (_I, [_P, _I, _P, _L, _L, _P, _P, _P, _P, _I]),
    "wfl_resample_workspace_bytes": (_L, [_I, _I]),
    "wfl_resample_pcm16": (_I, [_P, _L, _P, _P, _I, _I, _I, _P, _L, _I, _P, _L, _P]),
    "wfl_boundary_workspace_bytes": (_L, [_I, _I]),
    "wfl_boundary_features": (_I, [_P, _L, _P, _I, _I, _P, _P, _P, _P, _P, _L, _P]),
    "wfl_align_workspace_bytes": (_L, [_P, _P, _I]),
    "wfl_align": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P, _P, _P, _P, _P]),
    "wfl_align_windowed": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P, _P, _P, _P, _P]),
    "wfl_align_min_duration": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P, _P, _P, _P, _P]),
    "wfl_align_optional_workspace_bytes": (_L, [_P, _P, _I]),
    "wfl_align_optional": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _F, _P, _L, _P, _P, _P, _P, _P, _P]),
    "wfl_align_filler_workspace_bytes": (_L, [_P, _P, _I]),
    "wfl_align_filler": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _F, _P, _L, _P, _P, _P, _P, _P]),
    "wfl_align_graph_workspace_bytes": (_L, [_P, _P, _I]),
    "wfl_align_graph": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _L, _P, _P, _P, _P, _P, _P]),
    "wfl_align_duration_prior_workspace_bytes": (_L, [_P, _P, _I, _I]),
    "wfl_align_duration_prior": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _L, _P, _P, _P, _P, _P]),
    "wfl_align_duration_prior_posterior_workspace_bytes": (_L, [_P, _P, _I, _I]),
    "wfl_align_duration_prior_posterior": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _P, _L,
                                                 _P, _P, _P, _P, _P, _P, _P, _P]),
    "wfl_align_duration_prior_counts_workspace_bytes": (_L, [_P, _P, _I, _I]),
    "wfl_align_duration_prior_counts": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _L, _P, _P, _P, _P]),
    "wfl_align_posterior_workspace_bytes": (_L, [_P, _P, _I]),
    "wfl_align_posterior": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _L, _P, _P, _P, _P, _P, _P]),
    "wfl_align_posterior_windowed": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _L, _P, _P, _P, _P, _P, _P]),
    "wfl_align_min_duration_posterior_workspace_bytes": (_L, [_P, _P, _I]),
    "wfl_align_min_duration_posterior": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _L, _P, _P, _P, _P, _P, _P]),
    "wfl_align_optional_posterior_workspace_bytes": (_L, [_P, _P, _I]),
    "wfl_align_optional_posterior": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _F, _P, _P, _L, _P, _P, _P, _P, _P, _P,
                                          _P]),
    "wfl_align_filler_posterior_workspace_bytes": (_L, [_P, _P, _I]),
    "wfl_align_filler_posterior": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _F, _P, _P, _L, _P, _P, _P, _P, _P, _P,
                                        _P, _P]),
    "wfl_align_edits_workspace_bytes": (_L, [_P, _P, _I]),
    "wfl_align_edits": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _L, _P, _P, _P, _P]),
    "wfl_align_insertions_workspace_bytes": (_L, [_P, _P, _I]),
    "wfl_align_insertions": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _L, _P, _P, _P, _P]),
    "wfl_decode_workspace_bytes": (_L, [_P, _I, _I]),
    "wfl_decode": (_I, [_P, _L, _I, _I, _P, _P, _I, _P, _I, _F, _F, _P, _L, _P, _P, _P, _P]),
    "wfl_decode_posterior_workspace_bytes": (_L, [_P, _I, _I]),
    "wfl_decode_posterior": (_I, [_P, _L, _I, _I, _P, _P, _I, _P, _I, _F, _F, _P, _P, _L, _P, _P, _P, _P, _P]),
    "wfl_decode_bigram_workspace_bytes": (_L, [_P, _I, _I]),
    "wfl_decode_bigram": (_I, [_P, _L, _I, _I, _P, _P, _I, _P, _I, _P, _F, _P, _L, _P, _P, _P, _P]),
    "wfl_decode_bigram_posterior_workspace_bytes": (_L, [_P, _I, _I]),
    "wfl_decode_bigram_posterior": (_I, [_P, _L, _I, _I, _P, _P, _I, _P, _I, _P, _F, _P, _P, _L, _P, _P, _P, _P, _P]),
    "wfl_decode_bigram_counts_workspace_bytes": (_L, [_P, _I, _I]),
    "wfl_decode_bigram_counts": (_I, [_P, _L, _I, _I, _P, _P, _I, _P, _I, _P, _F, _P, _L, _P, _P, _P, _P]),
    "wfl_decode_duration_workspace_bytes": (_L, [_P, _I, _I, _I]),
    "wfl_decode_duration": (_I, [_P, _L, _I, _I, _P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _F, _P, _L, _P, _P, _P, _P]),
    "wfl_decode_duration_posterior_workspace_bytes": (_L, [_P, _I, _I, _I]),
    "wfl_decode_duration_posterior": (_I, [_P, _L, _I, _I, _P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _F, _P, _P, _L, _P, _P, _P, _P, _P]),
    "wfl_decode_duration_counts_workspace_bytes": (_L, [_P, _I, _I, _I]),
    "wfl_decode_duration_counts": (_I, [_P, _L, _I, _I, _P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _F, _P, _L, _P, _P, _P, _P, _P]),
    "wfl_gemm_profile_enable":(_I, [_P, _I]),
    "wfl_gemm_profile_read": (_I, [_P, _I, _P, _P, _P, _P, _P, _I]),
}

_lib = None


class WflError(RuntimeError):
    pass


def load():
    """dlopen the in-tree library (import torch first so both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WflError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.wfl_abi_version() != ABI_VERSION:
        raise WflError("libwfl_asr_hip.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


def ptr(t):
    """A device tensor's address for the C ABI (None: a null pointer)."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def host_ptr(a):
    """A contiguous numpy array's address for the C ABI."""
    return a.ctypes.data_as(C.c_void_p)


def back_to_back(n_frames):
    """The default `frame_offsets` of a ragged batch: the clips' rows one after the other (int64)."""
    T = np.asarray(n_frames, np.int64).reshape(-1)
    return np.concatenate([[0], np.cumsum(T)[:-1]]) if T.size else np.zeros(0, np.int64)


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().wfl_last_error()
        raise WflError(f"{what}: {msg.decode() if msg else rc}")
