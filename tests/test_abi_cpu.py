"""CPU: the C-ABI library builds, loads, matches the header struct sizes, and exports every function that
include/usdm_hip.h declares; the drop-in import paths resolve; CPU tensors are refused (no fallback)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from usdm_amd import _lib
    pat = r"^(?:int|int64_t|void\*|const char\*|const usdm_p2p_dev\*)\s+(usdm_\w+)\s*\("
    hdr = open(os.path.join(ROOT, "include", "usdm_hip.h")).read()
    names = set(re.findall(pat, hdr, flags=re.M))
    assert len(names) >= 40 and "usdm_allreduce_p2p_create" in names and "usdm_allreduce_p2p_bytes" in names, names
    assert {"usdm_gemm", "usdm_gemm_tile_for", "usdm_gemm_tile_info"} <= names, names
    # opt-in kernels that measured slower than the default live in their own header, outside the stable C-ABI
    exp = set(re.findall(pat, open(os.path.join(ROOT, "include", "usdm_hip_experimental.h")).read(), flags=re.M))
    assert exp == {"usdm_gemv_chain", "usdm_gemv_engine"} and not (exp & names), exp
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in sorted(names) if not hasattr(lib, n)]
    assert not missing, missing
    assert _lib.lib.usdm_abi_version() >= 1
    # ... and in their own BINARY (round 4): the product library does not carry them, libusdm_hip_experimental.so does
    assert not [n for n in sorted(exp) if hasattr(lib, n)], "experimental kernels leaked into the product library"
    elib = _lib.exp()
    assert not [n for n in sorted(exp) if not hasattr(elib, n)]


def test_bad_arguments_are_reported_not_crashed():
    from usdm_amd import _lib
    a = _lib.GemmArgs()
    rc = _lib.lib.usdm_gemm(ctypes.byref(a), ctypes.c_void_p(0))
    assert rc == 2 and b"usdm_gemm" in _lib.lib.usdm_last_error()
    with pytest.raises(_lib.UsdmError):
        _lib.check(rc, "usdm_gemm")


def test_dropin_paths_and_no_cpu_fallback():
    import usdm_amd.dropin as D
    D.install()
    from seamless_communication.models.unit_extractor import UnitExtractor  # noqa: F401
    from voicebox.model import Voicebox  # noqa: F401
    from voicebox.util.model_util import initialize_decoder, mel_mean, mel_std, process_unit, reconstruct_speech  # noqa: F401
    from voicebox.vocoder.models import BigVGAN  # noqa: F401
    assert (mel_mean, mel_std) == (-5.5419, 2.1575)
    from usdm_amd import _lib, ops
    with pytest.raises(_lib.UsdmError):
        ops.process_unit(torch.zeros(4, dtype=torch.int64), 441, 256)
    from usdm_amd.llm import USDMForCausalLM
    with pytest.raises(RuntimeError):
        USDMForCausalLM(dict(head_dim=128), "cpu")


def test_inference_helpers_match_reference_semantics():
    from usdm_amd.inference import default_template, generate_bad_words_ids, strip_exact_multiple
    t = default_template("<|unit1|>", "hi", "yo")
    assert t.endswith("<|unit1|><|correspond|>hi\n### Agent\nyo<|correspond|>") and t.startswith("Below is a conversation")
    assert strip_exact_multiple("\n hi \n", ["\n", " "]) == "hi"
    assert strip_exact_multiple("  hi", [" "]) == " hi"  # one occurrence per pattern, as the reference
    b = generate_bad_words_ids(0, 32002, exclude=[28705])
    assert len(b) == 32001 and [28705] not in b and b[0] == [0] and b[-1] == [32001]
    from oracle.units_oracle import banned_ranges
    ids = {w[0] for w in b}
    assert ids == {i for lo, hi in banned_ranges("text2unit") for i in range(lo, hi)}


def test_p2p_buffer_layout_arithmetic():
    """usdm_allreduce_p2p_*: one rank's exchange buffer = 256-byte header + [parity 2][site][src 8][elem] 8-byte granules;
    the 7B decode needs 2*32+1 sites of 4096 elements = 34 MB per rank."""
    from usdm_amd import p2p
    assert p2p.lib.usdm_allreduce_p2p_bytes(ctypes.c_int32(65), ctypes.c_int32(4096)) == 256 + 2 * 65 * 8 * 4096 * 8
    assert p2p.lib.usdm_allreduce_p2p_bytes(ctypes.c_int32(1), ctypes.c_int32(2)) == 256 + 2 * 8 * 2 * 8
    # no GPU here: creating a communicator must fail with an error code and a message, not crash
    h = ctypes.c_void_p()
    rc = p2p.lib.usdm_allreduce_p2p_create(ctypes.c_int32(0), ctypes.c_int32(9), ctypes.c_int32(1), ctypes.c_int32(2), ctypes.c_int32(10), ctypes.byref(h))
    assert rc == 2 and b"world" in p2p.lib.usdm_last_error()


def test_gemv_threads_table():
    """usdm_gemv_threads = 64 x the waves of the one launch selection (csrc/gemv_launch.h gemv_select): the table for the shapes
    the project runs.  usdm_gemv_engine reproduces the RMSNorm partition from it."""
    from usdm_amd import _lib
    f = _lib.lib.usdm_gemv_threads

    def threads(N, K=4096, **kw):
        a = _lib.GemvArgs(N=N, K=K, ldw=K, **kw)
        return f(ctypes.byref(a))

    assert threads(6144) == 768                                        # 24 rows per CU: 2 x 12 waves
    assert threads(4096) == 1024 and threads(4096, K=14336) == 1024    # 16 rows per CU: 1 x 16 waves
    assert threads(28672, act=3) == 448                                # gate/up of the 7B: 14 outputs per 7-wave workgroup
    assert threads(42003, part_val=8, part_idx=8) == 256               # lm_head: 4 rows x 4 waves
    for kw in (dict(mrg_po=8), dict(p2p_mode=1), dict(mrg_po=8, p2p_mode=1)):
        assert threads(4096, **kw) == 1024 and threads(1024, **kw) == 256
    assert threads(1000) == 256                                        # no special row: the balance rule's pick, 4 waves
