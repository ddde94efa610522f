"""ctypes binding of libusdm_hip.so (C-ABI declared in include/usdm_hip.h).

No fallback: if the shared library is missing or an entry point is absent this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libusdm_hip.so")


class UsdmError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build it with `python -m usdm_amd.build` (hipcc --offload-arch=gfx950). "
        "usdm_amd has no CPU fallback.")

lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)      # (global: the experimental library resolves usdm_set_error here)
lib.usdm_last_error.restype = C.c_char_p
lib.usdm_gemv_batch_ks_floats.restype = C.c_int64
lib.usdm_gemm_tile_info.restype = C.c_int    # (the tile table's query: resolving it here makes a stale library fail at import)
lib.usdm_gemv_fp8_mfma.restype = C.c_int     # (the FP8 matrix-core form; resolving it here makes a stale library fail at import)
lib.usdm_attn_decode_fp8.restype = C.c_int   # (the FP8 KV cache entry points: likewise)
lib.usdm_rope_cache_fp8.restype = C.c_int
lib.usdm_gemv_mxfp4.restype = C.c_int        # (the MXFP4 entry points: likewise)
lib.usdm_dequant_mxfp4.restype = C.c_int
lib.usdm_gemv_mxfp4_mfma.restype = C.c_int   # (the MXFP4 matrix-core form: likewise)
lib.usdm_gemv_packed.restype = C.c_int       # (the 13-bit weight image: likewise)
lib.usdm_gemv_packs.restype = C.c_int
lib.usdm_gemv_packed_glu.restype = C.c_int   # (its gate/up form: likewise)
lib.usdm_gemv_packs_glu.restype = C.c_int
lib.usdm_logprobs.restype = C.c_int          # (the log-probability entry points: likewise)
lib.usdm_logprobs_seg.restype = C.c_int
lib.usdm_prompt_logprobs.restype = C.c_int   # (the scoring entry points: likewise)
lib.usdm_prompt_logprobs_seg.restype = C.c_int
lib.usdm_penalize.restype = C.c_int          # (the penalty entry points: likewise)
lib.usdm_penalize_seg.restype = C.c_int
lib.usdm_penalty_params_init.restype = C.c_int
lib.usdm_logit_edit.restype = C.c_int        # (the logit-edit entry points: likewise)
lib.usdm_logit_edit_seg.restype = C.c_int
lib.usdm_beam_step.restype = C.c_int         # (the beam-search entry points: likewise)
lib.usdm_kv_reorder.restype = C.c_int
lib.usdm_kv_expand.restype = C.c_int         # (the prefix-cache entry point: likewise)
lib.usdm_attn_verify.restype = C.c_int       # (the speculative-decoding entry points: likewise)
lib.usdm_spec_commit.restype = C.c_int
lib.usdm_attn_verify_batch.restype = C.c_int
lib.usdm_spec_commit_batch.restype = C.c_int
lib.usdm_spec_sample.restype = C.c_int       # (sampled speculation: the rows' draws and the commit from given picks)
lib.usdm_spec_commit_picks.restype = C.c_int
lib.usdm_spec_commit_batch_picks.restype = C.c_int
_exp = None


def exp():
    """libusdm_hip_experimental.so (include/usdm_hip_experimental.h): kernels that measured slower than the default path, kept out of
    the product library; loaded on first use by ops.gemv_chain / ops.gemv_engine only."""
    global _exp
    if _exp is None:
        path = os.path.join(_HERE, "libusdm_hip_experimental.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} not found: build it with `python -m usdm_amd.build`")
        e = C.CDLL(path)
        n = e.usdm_sizeof_gemv_chain_args()
        if n != C.sizeof(GemvChainArgs):
            raise ImportError(f"ABI mismatch: usdm_gemv_chain_args is {n} bytes in the library, {C.sizeof(GemvChainArgs)} in Python")
        _exp = e
    return _exp

BF16, F32 = 0, 1
ACT_NONE, ACT_GELU, ACT_SWIGLU, ACT_TANH, ACT_LOGCLAMP = 0, 1, 3, 4, 5
EPI_PLAIN, EPI_QKV_HEADS = 0, 1


class GemmArgs(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("taps", C.c_int32), ("Kc", C.c_int32),
        ("A", C.c_void_p), ("lda", C.c_int64), ("rowsA", C.c_int32),
        ("a_row_mul", C.c_int32), ("a_row_off", C.c_int32), ("a_row_step", C.c_int32),
        ("a_tap_stride", C.c_int64),
        ("W", C.c_void_p), ("ldw", C.c_int64),
        ("groups", C.c_int32), ("batch", C.c_int32),
        ("a_gstride", C.c_int64), ("w_gstride", C.c_int64), ("a_bstride", C.c_int64),
        ("c_gcol", C.c_int32), ("c_bstride", C.c_int64),
        ("bias", C.c_void_p), ("alpha", C.c_float), ("act", C.c_int32), ("round_bf16", C.c_int32),
        ("residual", C.c_void_p), ("res_dtype", C.c_int32), ("ldr", C.c_int64),
        ("C32", C.c_void_p), ("C16", C.c_void_p), ("ldc", C.c_int64),
        ("c_row_mul", C.c_int32), ("c_row_off", C.c_int32), ("transpose_out", C.c_int32), ("epi", C.c_int32),
        ("qkv_S", C.c_int32), ("qkv_Spad", C.c_int32), ("qkv_H", C.c_int32), ("qkv_D", C.c_int32),
        ("qkv_q", C.c_void_p), ("qkv_k", C.c_void_p), ("qkv_v", C.c_void_p),
        ("split_k", C.c_int32), ("c_split_stride", C.c_int64),
        ("stats_out", C.c_void_p), ("ln_stats", C.c_void_p), ("ln_nt", C.c_int32), ("ln_mode", C.c_int32), ("ln_C", C.c_int32),
        ("ln_eps", C.c_float), ("ln_c", C.c_void_p), ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p),
        ("ln_guard", C.c_void_p), ("ln_guard_ratio", C.c_float), ("tile_sel", C.c_int32),
    ]


class NormArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x_dtype", C.c_int32), ("ldx", C.c_int64),
        ("res", C.c_void_p), ("res_dtype", C.c_int32), ("ldr", C.c_int64),
        ("gamma", C.c_void_p), ("beta", C.c_void_p), ("eps", C.c_float),
        ("rows", C.c_int32), ("C", C.c_int32),
        ("rms", C.c_int32), ("act", C.c_int32), ("round_bf16", C.c_int32), ("premask", C.c_int32),
        ("valid_len", C.c_void_p), ("rows_per_batch", C.c_int32),
        ("out32", C.c_void_p), ("out16", C.c_void_p), ("ldo", C.c_int64),
        ("sum32", C.c_void_p), ("sum16", C.c_void_p), ("lds", C.c_int64),
        ("res2", C.c_void_p), ("n_res2", C.c_int32), ("res2_stride", C.c_int64),
    ]


class SnakeArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int64),
        ("T", C.c_int32), ("C", C.c_int32), ("Creal", C.c_int32), ("L", C.c_int32),
        ("alpha", C.c_void_p), ("beta", C.c_void_p), ("logscale", C.c_int32),
        ("fup", C.c_float * 12), ("fdn", C.c_float * 12),
        ("out32", C.c_void_p), ("out16", C.c_void_p), ("ldo", C.c_int64),
    ]


class AttnArgs(C.Structure):
    _fields_ = [
        ("mode", C.c_int32), ("dh", C.c_int32), ("B", C.c_int32), ("Hq", C.c_int32), ("Hkv", C.c_int32),
        ("Sq", C.c_int32), ("Skv", C.c_int32), ("Skv_alloc", C.c_int32), ("q_pos0", C.c_int32),
        ("alibi_col0_zero", C.c_int32), ("scale", C.c_float), ("head_order", C.c_int32),
        ("q", C.c_void_p), ("q_bs", C.c_int64), ("q_hs", C.c_int64), ("q_rs", C.c_int64),
        ("k", C.c_void_p), ("k_bs", C.c_int64), ("k_hs", C.c_int64), ("k_rs", C.c_int64),
        ("vt", C.c_void_p), ("v_bs", C.c_int64), ("v_hs", C.c_int64), ("v_ds", C.c_int64),
        ("o", C.c_void_p), ("o_bs", C.c_int64), ("o_rs", C.c_int64),
        ("kv_len", C.c_void_p), ("slopes", C.c_void_p), ("window", C.c_int32), ("variant", C.c_int32),
    ]


class VbInputArgs(C.Structure):
    _fields_ = [
        ("ids", C.c_void_p), ("y", C.c_void_p), ("cond", C.c_void_p), ("table", C.c_void_p),
        ("B_in", C.c_int32), ("dup", C.c_int32), ("S", C.c_int32), ("E", C.c_int32), ("F", C.c_int32),
        ("null_id", C.c_int32), ("use_cond", C.c_int32),
        ("out", C.c_void_p), ("ldo", C.c_int64), ("out_dtype", C.c_int32),
    ]


class VbSolverArgs(C.Structure):
    _fields_ = [
        ("vout", C.c_void_p), ("z", C.c_void_p), ("v1", C.c_void_p), ("eps", C.c_void_p), ("cond", C.c_void_p),
        ("z_in", C.c_void_p), ("z_commit", C.c_void_p), ("t_cur", C.c_void_p),
        ("B", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("P", C.c_int32), ("cfg", C.c_int32), ("mode", C.c_int32),
        ("t_count", C.c_int32),
        ("gs", C.c_float), ("dt", C.c_float), ("c_eps", C.c_float), ("c_cond", C.c_float), ("t_next", C.c_float),
    ]


class GemvArgs(C.Structure):
    _fields_ = [
        ("W", C.c_void_p), ("ldw", C.c_int64), ("N", C.c_int32), ("K", C.c_int32),
        ("x", C.c_void_p), ("norm_w", C.c_void_p), ("eps", C.c_float),
        ("act", C.c_int32), ("round_bf16", C.c_int32),
        ("residual", C.c_void_p), ("y16", C.c_void_p), ("y32", C.c_void_p),
        ("ban", C.c_void_p), ("part_val", C.c_void_p), ("part_idx", C.c_void_p), ("idx_offset", C.c_int32),
        ("x_delta", C.c_void_p), ("x_out", C.c_void_p), ("skip", C.c_void_p),
        ("p2p", C.c_void_p), ("p2p_site", C.c_int32), ("p2p_mode", C.c_int32),
        ("mrg_pm", C.c_void_p), ("mrg_pl", C.c_void_p), ("mrg_po", C.c_void_p), ("mrg_ns", C.c_int32),
        ("cmb_gran", C.c_void_p), ("cmb_err", C.c_void_p), ("cmb_timeout_ms", C.c_int32),
        ("resident", C.c_int32),
    ]


class GemvChainArgs(C.Structure):
    _fields_ = [("ph", GemvArgs * 4), ("nph", C.c_int32), ("sync", C.c_void_p), ("timeout_ms", C.c_int32), ("gran", C.c_void_p),
                ("norm_nth", C.c_int32 * 4)]


class GemvBatchArgs(C.Structure):
    _fields_ = [
        ("g", GemvArgs), ("nb", C.c_int32), ("x_bs", C.c_int64), ("y_bs", C.c_int64), ("res_bs", C.c_int64), ("part_bs", C.c_int32),
        ("form", C.c_int32), ("ks_part", C.c_void_p), ("ks_cnt", C.c_void_p), ("ks_part_floats", C.c_int64),
    ]


class GemvFp8Args(C.Structure):
    _fields_ = [("b", GemvBatchArgs), ("row_exp", C.c_void_p)]


class GemvMxfp4Args(C.Structure):
    _fields_ = [("b", GemvBatchArgs), ("scales", C.c_void_p), ("lds", C.c_int64)]


class GemvMxfp4MfmaArgs(C.Structure):
    _fields_ = [("b", GemvBatchArgs), ("codes", C.c_void_p), ("ldc", C.c_int64), ("scales", C.c_void_p), ("lds", C.c_int64)]


class GemvMfmaPlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("hold", "cpwt", "trl", "rt", "ksplit", "ntiles", "nout", "cpw", "grid", "kwg", "lds_bytes")]


class DecodeState(C.Structure):
    _fields_ = [
        ("next_token", C.c_void_p), ("out_tokens", C.c_void_p), ("step", C.c_void_p), ("pos", C.c_void_p),
        ("max_out", C.c_int32), ("id_offset", C.c_int32), ("advance_pos", C.c_int32), ("batch", C.c_int32),
        ("done", C.c_void_p), ("eos", C.c_void_p),
    ]


class P2pDev(C.Structure):
    _fields_ = [("base", C.c_uint64 * 8), ("rank", C.c_int32), ("world", C.c_int32), ("n_sites", C.c_int32), ("max_elems", C.c_int32),
                ("timeout_ticks", C.c_uint64)]


class SampleParams(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("min_p", C.c_float), ("seed", C.c_uint64)]


class SampleArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("V", C.c_int32), ("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float),
        ("seed", C.c_uint64), ("probs_out", C.c_void_p), ("dev_params", C.c_void_p), ("logits_bs", C.c_int64),
        ("min_p", C.c_float),
    ]


class LogprobArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("V", C.c_int32), ("K", C.c_int32), ("logits_bs", C.c_int64),
        ("tok_lp", C.c_void_p), ("tok_rank", C.c_void_p), ("top_id", C.c_void_p), ("top_lp", C.c_void_p),
        ("tok_bs", C.c_int64), ("top_bs", C.c_int64), ("count", C.c_void_p),
    ]


class PromptLogprobArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("V", C.c_int32), ("K", C.c_int32), ("logits_bs", C.c_int64),
        ("ids", C.c_void_p), ("n_ids", C.c_int32), ("row0", C.c_int32), ("rows", C.c_int32),
        ("tok_lp", C.c_void_p), ("tok_rank", C.c_void_p), ("top_id", C.c_void_p), ("top_lp", C.c_void_p),
    ]


class PenaltyParams(C.Structure):
    _fields_ = [("repetition", C.c_float), ("frequency", C.c_float), ("presence", C.c_float), ("reserved", C.c_int32)]


class PenaltyArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("V", C.c_int32), ("logits_bs", C.c_int64), ("table", C.c_void_p), ("table_bs", C.c_int64),
        ("dev_params", C.c_void_p), ("count", C.c_void_p),
    ]


class LogitEditParams(C.Structure):
    _fields_ = [("ngram", C.c_int32), ("prompt_len", C.c_int32), ("n_bias", C.c_int32), ("reserved", C.c_int32)]


class LogitEditArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("V", C.c_int32), ("logits_bs", C.c_int64), ("dev_params", C.c_void_p),
        ("bias_id", C.c_void_p), ("bias_val", C.c_void_p), ("bias_max", C.c_int32), ("bias_bs", C.c_int64),
        ("prompt", C.c_void_p), ("prompt_max", C.c_int32), ("prompt_bs", C.c_int64),
    ]


class BeamArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("V", C.c_int32), ("logits_bs", C.c_int64), ("score", C.c_void_p), ("parent", C.c_void_p),
        ("nlive", C.c_int32), ("n_eos", C.c_int32), ("eos", C.c_void_p),
        ("log_score", C.c_void_p), ("log_token", C.c_void_p), ("log_parent", C.c_void_p), ("log_rows", C.c_int32),
        ("cand_score", C.c_void_p), ("cand_index", C.c_void_p),
    ]


class KvReorderArgs(C.Structure):
    _fields_ = [
        ("base", C.c_void_p * 4), ("slot_bytes", C.c_int64 * 4), ("row_bytes", C.c_int32 * 4),
        ("n_arrays", C.c_int32), ("nblk", C.c_int32), ("ctx_max", C.c_int32), ("B", C.c_int32),
        ("parent", C.c_void_p), ("lo", C.c_void_p), ("pos", C.c_void_p),
    ]


class KvExpandArgs(C.Structure):
    _fields_ = [
        ("kcache", C.c_void_p), ("vcache", C.c_void_p), ("kexp", C.c_void_p), ("vexp", C.c_void_p),
        ("kscr", C.c_void_p), ("kscr_ld", C.c_int64), ("vt", C.c_void_p), ("vt_ld", C.c_int64),
        ("Hkv", C.c_int32), ("ctx_max", C.c_int32), ("n", C.c_int32),
    ]


class RopeArgs(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("ld", C.c_int64), ("S", C.c_int32), ("pos0", C.c_int32), ("Hq", C.c_int32),
        ("Hkv", C.c_int32), ("ctx_max", C.c_int32), ("max_pos", C.c_int32),
        ("cos", C.c_void_p), ("sin", C.c_void_p),
        ("kcache", C.c_void_p), ("vcache", C.c_void_p), ("vt", C.c_void_p), ("vt_ld", C.c_int64),
    ]


class AttnDecodeArgs(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("pos", C.c_void_p),
        ("Hq", C.c_int32), ("Hkv", C.c_int32), ("ctx_max", C.c_int32), ("NS", C.c_int32), ("scale", C.c_float),
        ("cos", C.c_void_p), ("sin", C.c_void_p),
        ("kcache", C.c_void_p), ("vcache", C.c_void_p),
        ("pm", C.c_void_p), ("pl", C.c_void_p), ("po", C.c_void_p), ("out", C.c_void_p), ("counters", C.c_void_p),
        ("batch", C.c_int32), ("qkv_bs", C.c_int64), ("out_bs", C.c_int64), ("cache_bs", C.c_int64), ("skip", C.c_void_p),
        ("defer_merge", C.c_int32), ("window", C.c_int32), ("cmb_gran", C.c_void_p),
    ]


class AttnDecodeFp8Args(C.Structure):
    _fields_ = [("a", AttnDecodeArgs), ("kexp", C.c_void_p), ("vexp", C.c_void_p), ("exp_bs", C.c_int64)]


class RopeFp8Args(C.Structure):
    _fields_ = [("r", RopeArgs), ("kexp", C.c_void_p), ("vexp", C.c_void_p), ("kscr", C.c_void_p), ("kscr_ld", C.c_int64)]


class AttnVerifyArgs(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("qkv_ld", C.c_int64), ("pos", C.c_void_p),
        ("T", C.c_int32), ("Hq", C.c_int32), ("Hkv", C.c_int32), ("ctx_max", C.c_int32), ("C", C.c_int32), ("window", C.c_int32),
        ("scale", C.c_float),
        ("cos", C.c_void_p), ("sin", C.c_void_p), ("kcache", C.c_void_p), ("vcache", C.c_void_p),
        ("pm", C.c_void_p), ("pl", C.c_void_p), ("po", C.c_void_p), ("out", C.c_void_p), ("out_ld", C.c_int64), ("skip", C.c_void_p),
    ]


class SpecArgs(C.Structure):
    _fields_ = [
        ("part_val", C.c_void_p), ("part_idx", C.c_void_p), ("nparts", C.c_int32), ("T", C.c_int32),
        ("drafts", C.c_void_p), ("limit", C.c_void_p),
        ("prompt", C.c_void_p), ("prompt_len", C.c_void_p), ("prompt_max", C.c_int32),
        ("script", C.c_void_p), ("params", C.c_void_p), ("V", C.c_int32), ("counters", C.c_void_p), ("propose_only", C.c_int32),
    ]


class AttnVerifyBatchArgs(C.Structure):
    _fields_ = [("v", AttnVerifyArgs), ("B", C.c_int32), ("cache_bs", C.c_int64)]


class SpecBatchArgs(C.Structure):
    _fields_ = [("s", SpecArgs), ("slot_lo", C.c_int32), ("n", C.c_int32)]


class SpecSampleArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("logits_bs", C.c_int64), ("V", C.c_int32), ("T", C.c_int32), ("n", C.c_int32),
        ("dev_params", C.c_void_p), ("step", C.c_void_p), ("done", C.c_void_p), ("drafts", C.c_void_p), ("picks", C.c_void_p),
    ]


def check(rc, what=""):
    if rc != 0:
        raise UsdmError(f"{what} failed (rc={rc}): {lib.usdm_last_error().decode()}")


def _selfcheck():
    assert lib.usdm_abi_version() >= 1
    n = lib.usdm_sizeof_gemm_args()
    if n != C.sizeof(GemmArgs):
        raise ImportError(f"ABI mismatch: usdm_gemm_args is {n} bytes in the library, {C.sizeof(GemmArgs)} in Python")
    for name, cls in (("norm", NormArgs), ("snake", SnakeArgs), ("attn", AttnArgs), ("vb_input", VbInputArgs),
                      ("vb_solver", VbSolverArgs), ("gemv", GemvArgs), ("decode_state", DecodeState),
                      ("rope", RopeArgs), ("attn_decode", AttnDecodeArgs), ("sample", SampleArgs),
                      ("gemv_batch", GemvBatchArgs), ("gemv_fp8", GemvFp8Args), ("gemv_mxfp4", GemvMxfp4Args), ("p2p_dev", P2pDev),
                      ("gemv_mxfp4_mfma", GemvMxfp4MfmaArgs),
                      ("attn_decode_fp8", AttnDecodeFp8Args), ("rope_fp8", RopeFp8Args), ("logprob", LogprobArgs),
                      ("penalty", PenaltyArgs), ("logit_edit", LogitEditArgs), ("prompt_logprob", PromptLogprobArgs), ("beam", BeamArgs),
                      ("kv_reorder", KvReorderArgs), ("kv_expand", KvExpandArgs), ("attn_verify", AttnVerifyArgs), ("spec", SpecArgs),
                      ("attn_verify_batch", AttnVerifyBatchArgs), ("spec_batch", SpecBatchArgs),
                      ("spec_sample", SpecSampleArgs)):
        n = getattr(lib, f"usdm_sizeof_{name}" if name in ("decode_state", "p2p_dev") else f"usdm_sizeof_{name}_args")()
        if n != C.sizeof(cls):
            raise ImportError(f"ABI mismatch: usdm_{name}_args is {n} bytes in the library, {C.sizeof(cls)} in Python")
    if lib.usdm_sizeof_penalty_params() != C.sizeof(PenaltyParams):
        raise ImportError("ABI mismatch: usdm_penalty_params")
    if lib.usdm_sizeof_logit_edit_params() != C.sizeof(LogitEditParams):
        raise ImportError("ABI mismatch: usdm_logit_edit_params")
    if lib.usdm_sizeof_gemv_mfma_plan() != C.sizeof(GemvMfmaPlan):
        raise ImportError("ABI mismatch: usdm_gemv_mfma_plan")


_selfcheck()
