"""The single-sequence decode step with down_proj streamed from the lossless 13-bit weight image (usdm_amd/wpack.py; default on)
against the same model with USDM_WPACK=0: MISTRAL_7B_USDM cut to 2 layers, random init.  16 greedy tokens from a 32-token prompt:
the token ids and the bits of the last step's logits are equal, and the packed model's decode plan really holds packed launches."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _packed_launches(m):
    from usdm_amd import _lib, ops
    calls = [c for s in m._build_decode() if isinstance(s, ops.Plan) for c in s.calls if c[0] == "usdm_gemv"]
    packed = [c for c in calls if c[1].__name__ == "usdm_gemv_packed"]
    for what, fn, args in packed:
        a = args[0]._obj
        assert (a.N, a.K, a.act) == (4096, 14336, 0) and _lib.lib.usdm_gemv_packs(ctypes.byref(a)) == 1
    return len(packed), len(calls)


def test_tokens_and_logits_equal_with_and_without_the_image(dev, monkeypatch):
    from usdm_amd.llm import MISTRAL_7B_USDM, USDMForCausalLM
    cfg = dict(MISTRAL_7B_USDM, num_hidden_layers=2)
    ids = torch.randint(0, 42003, (1, 32), generator=torch.Generator().manual_seed(32)).to(dev)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("USDM_WPACK", flag)
        m = USDMForCausalLM.random_init(cfg, dev, seed=5, ctx_max=256)
        assert m.weight_packing == (flag == "1")
        npacked, ngemv = _packed_launches(m)
        if flag == "1":
            r = m.wpack_report
            print(f"marked rows {r['down_marked_rows']} of {2 * 4096}, image {r['extra_bytes']} bytes, packed in {r['seconds']:.2f} s")
            assert npacked == 2 and ngemv == 4 * 2 + 1 and r["extra_bytes"] == 2 * (4096 * 7 * 3328 + 4096)
            assert all(s < 0.02 for s in r["down_marked_share"])
        else:
            assert npacked == 0 and m.wpack_down is None and m.wpack_report is None
        m.keep_logits = True
        o = m.generate(input_ids=ids, max_new_tokens=16)
        out[flag] = (o[0].tolist(), m.last_logits.clone().cpu())
        del m
        torch.cuda.empty_cache()
    assert len(out["1"][0]) >= 16 and out["1"][0] == out["0"][0]
    assert torch.equal(out["1"][1].view(torch.int32), out["0"][1].view(torch.int32))
    # the keyword overrides the environment
    m = USDMForCausalLM.random_init(cfg, dev, seed=5, ctx_max=256, weight_packing=True)
    assert m.weight_packing and _packed_launches(m)[0] == 2
