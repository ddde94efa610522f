"""The single-sequence decode step with gate/up streamed from the lossless 13-bit weight image (usdm_amd/wpack.py; default on)
against the same model with USDM_WPACK_GU=0 (down_proj's image only): MISTRAL_7B_USDM cut to 2 layers, random init.  16 greedy
tokens from a 32-token prompt: the token ids and the bits of the last step's logits are equal, and the decode plan holds the two
gate/up launches through usdm_gemv_packed_glu beside the two down_proj launches through usdm_gemv_packed."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _packed_launches(m):
    from usdm_amd import _lib, ops
    calls = [c for s in m._build_decode() if isinstance(s, ops.Plan) for c in s.calls if c[0] == "usdm_gemv"]
    gu = [c for c in calls if c[1].__name__ == "usdm_gemv_packed_glu"]
    for what, fn, args in gu:
        a = args[0]._obj
        assert (a.N, a.K, a.act) == (28672, 4096, 3) and _lib.lib.usdm_gemv_packs_glu(ctypes.byref(a)) == 1
    return len(gu), len([c for c in calls if c[1].__name__ == "usdm_gemv_packed"]), len(calls)


def test_tokens_and_logits_equal_with_and_without_the_gate_up_image(dev, monkeypatch):
    from usdm_amd.llm import MISTRAL_7B_USDM, USDMForCausalLM
    cfg = dict(MISTRAL_7B_USDM, num_hidden_layers=2)
    ids = torch.randint(0, 42003, (1, 32), generator=torch.Generator().manual_seed(32)).to(dev)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("USDM_WPACK_GU", flag)
        m = USDMForCausalLM.random_init(cfg, dev, seed=5, ctx_max=256)
        assert m.weight_packing and m.weight_packing_gu == (flag == "1")
        ngu, ndown, ngemv = _packed_launches(m)
        r = m.wpack_report
        assert ndown == 2 and ngemv == 4 * 2 + 1 and r["extra_bytes"] == 2 * (4096 * 7 * 3328 + 4096)
        if flag == "1":
            print(f"marked gate/up outputs {r['gu_marked_outputs']} of 14336 each, image {r['gu_extra_bytes']} bytes, "
                  f"packed in {r['gu_seconds']:.2f} s")
            assert ngu == 2 and r["gu_extra_bytes"] == 2 * (28672 * 2 * 3328 + 28672)
            assert all(n < 0.02 * 14336 for n in r["gu_marked_outputs"])
        else:
            assert ngu == 0 and m.wpack_gu is None and "gu_extra_bytes" not in r
        m.keep_logits = True
        o = m.generate(input_ids=ids, max_new_tokens=16)
        out[flag] = (o[0].tolist(), m.last_logits.clone().cpu())
        del m
        torch.cuda.empty_cache()
    assert len(out["1"][0]) >= 16 and out["1"][0] == out["0"][0]
    assert torch.equal(out["1"][1].view(torch.int32), out["0"][1].view(torch.int32))
