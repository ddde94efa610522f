#!/usr/bin/env python3
"""Headline benchmark: end-to-end real-time factor + LLM tokens/s of the USDM inference hot path on MI355X.

One "step" = one synthetic 10 s utterance through the whole path with inputs resident in HBM:
  16 kHz wave (160 000 samples) -> XLS-R/k-means units (499) -> 7B LLM, three greedy rounds as src/inference.py:61-83
  (unit->text 32 tok, text->text 32 tok, text->unit 500 tok; EOS disabled so the step count is fixed) ->
  process_unit (500 -> 861 frames) -> Token-Voicebox, 64 "timesteps" Heun = 63 NFE with CFG and a 3 s speech
  prompt -> BigVGAN -> 220 416 samples of 22.05 kHz audio (9.996 s).
Random-init weights of the exact architectures (no network), synthetic data.
N > 1: the LLM runs tensor-parallel over N ranks (RCCL all-reduce); tokenizer / Voicebox / vocoder are replicated
(they do not shard within one utterance) -> strong scaling of ONE utterance; value = RTF of the whole job.

Prints ONE JSON line on rank 0 (measurement contract: BASELINE.md).  A plain run sets up, warms up, times --steps steps and
reports the headline figures of the timed steps only.  --full adds the measurements that take runs of their own:
  stage_rooflines : MFMA-bound stages against their peaks (one extra vocoder pass)
  roofline        : the dominant kernel (decode GEMV, HBM-bound) measured live with HIP events
  llm_batched_decode, pipeline_throughput : informational batched runs (single-rank runs only)
  cpu_baseline    : the CPU oracle timed on the host cores over a bounded sample, extrapolated (stated in "sample")
--dump-outputs DIR writes what the last timed step computed (audio + token ids) as DIR/<name>.npy, so that two builds can be
compared output for output: every input and weight is generated from fixed seeds.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "end-to-end real-time factor + LLM tokens/sec, 10 s utterance, 7B TP=1/8"
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--units", type=int, default=500, help="generated unit tokens (50 Hz) in the TTS round")
    ap.add_argument("--text-tokens", type=int, default=32)
    ap.add_argument("--nt", type=int, default=64, help="Voicebox n_timesteps (Heun halves it)")
    ap.add_argument("--full", action="store_true",
                    help="also measure stage rooflines, the decode-GEMV roofline, batched decode / pipeline throughput and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-batched", action="store_true", help="with --full: skip the informational batched-decode measurement")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--vocoder-dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--force-dist", action="store_true",
                    help="debug: run the multi-rank code path (process group, collectives, TP plan segments) on however many ranks there are")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


class Pipeline:
    def __init__(self, dev, rank, world, group, args):
        from usdm_amd import synth
        from usdm_amd.voicebox.util import model_util
        self.mu = model_util
        self.dev, self.rank, self.world, self.args = dev, rank, world, args
        t0 = time.time()
        self.ue = synth.make_unit_extractor(dev)
        # Tensor-parallel decode transport: one-shot peer-to-peer exchange fused into the GEMV epilogues (default), RCCL
        # through torch.distributed as the fallback.  The transport is CHECKED on the real ranks before it is trusted
        # (usdm_amd.p2p.self_test): if the check fails on this node the bench falls back to RCCL and says so in its JSON line.
        self.tp_comm, comm = "none", None
        tp_kw = dict(ctx_max=1536, tp_rank=rank, tp_size=world, group=group, tp_segments=True if (args.force_dist or world > 1) else None)
        if world > 1 or args.force_dist:
            self.tp_comm = "rccl"
            if os.environ.get("USDM_TP_COMM", "p2p") == "p2p":
                from usdm_amd.llm import MISTRAL_7B_USDM as C7
                from usdm_amd.p2p import P2PComm, self_test
                # Every step below ends in a verdict that is IDENTICAL on all ranks (usdm_amd.p2p.try_from_process_group / agree):
                # no rank ever leaves the group's collective sequence on its own.
                fused = os.environ.get("USDM_P2P_FUSED", "1") == "1"
                probe, why = P2PComm.try_from_process_group(group, 3, 4096, timeout_ms=3000)
                if probe is not None:
                    why = self_test(probe, group, dev, fused=fused)
                    probe.close(group)
                if why is None:
                    comm, why = P2PComm.try_from_process_group(group, 2 * C7["num_hidden_layers"] + 1, C7["hidden_size"])
                if why is not None:
                    self.tp_comm = f"rccl (p2p start-up check failed: {why})"
        self.llm = synth.make_llm(dev, p2p=comm, **tp_kw)
        if comm is not None:
            # in-situ check on the real model and the real ranks before the transport is trusted with the timed region: 24 greedy
            # tokens; every rank must hold the SAME token stream (the exchange sums in rank order on every rank, so any
            # difference means lost or stale partials) and a clean error word.  Otherwise: RCCL, same weights.
            why = self._tp_crosscheck(group)
            if why is None:
                self.tp_comm = ("p2p (one-shot xGMI exchange fused into the row-parallel GEMV epilogues; start-up self-test and "
                                "cross-rank token agreement passed on this node)" if fused else
                                "p2p, split form (put in the GEMV epilogue + reduce launch; self-test and token agreement passed)")
            else:
                from usdm_amd.llm import USDMForCausalLM
                W, old = self.llm.W, self.llm
                self.llm = USDMForCausalLM(old.cfg, dev, p2p=None, **tp_kw)
                self.llm.W = W
                self.llm._alloc()
                del old
                comm.close(group)
                self.tp_comm = f"rccl (p2p in-situ check failed: {why})"
        # Voicebox: the two classifier-free-guidance halves of every NFE on a PAIR of ranks (optional row): ranks
        # (2i, 2i+1) evaluate the unconditional / conditional estimator at batch 1 and all-gather the [1,80,S] velocities, instead
        # of every rank repeating the batch-2 estimator.  Even world sizes only; USDM_VB_CFG_SPLIT=0 switches it off.
        self.cfg_group, self.vb_mode = None, "replica (CFG batch 2 on every rank)"
        if world > 1 and world % 2 == 0 and os.environ.get("USDM_VB_CFG_SPLIT", "1") == "1":
            import torch.distributed as dist
            for i in range(0, world, 2):                      # every rank creates every pair group (new_group is collective)
                g2 = dist.new_group([i, i + 1])
                if rank in (i, i + 1):
                    self.cfg_group = g2
            self.vb_mode = "CFG halves on rank pairs (2i: unconditional, 2i+1: conditional), one all-gather per NFE"
        self.vb = synth.make_voicebox(dev)
        self.voc = synth.make_bigvgan(dev, compute_dtype=torch.float32 if args.vocoder_dtype == "f32" else torch.bfloat16)
        torch.cuda.synchronize()
        self.build_s = time.time() - t0
        g = torch.Generator().manual_seed(1)
        t = torch.arange(160000) / 16000.0
        wave = sum(torch.sin(2 * torch.pi * f * t + p) for f, p in zip((110, 220, 450, 900, 1800, 3100, 4700, 6100), torch.rand(8, generator=g) * 6.28))
        self.wave = (0.05 * wave + 0.02 * torch.randn(160000, generator=g)).float().to(dev)
        self.template_ids = torch.randint(3, 32000, (48,), generator=g)   # stand-in for the tokenised template text
        self.sep_ids = torch.randint(3, 32000, (6,), generator=g)         # "\n### Agent\n"
        self.ref_units = torch.randint(0, 10000, (149,), generator=g).to(dev)  # 3 s prompt
        self.ref_mel = (torch.randn(1, 80, 256, generator=g) * 2.1575 - 5.5419).to(dev)
        n_noise = 1 + (2 * ((args.nt + 1) // 2) - 1)
        self.frames = (args.units * 441) // 256
        self.noise = torch.randn(n_noise, 1, 80, 256 + self.frames, generator=g).to(dev)  # caller-supplied draws
        from usdm_amd.inference import generate_bad_words_ids
        self.bad_u2t = generate_bad_words_ids(32000, 42003)
        self.bad_t2t = generate_bad_words_ids(32002, 42003)
        self.bad_t2u = generate_bad_words_ids(0, 32002, exclude=[28705])
        self.ev = {}

    def _tp_crosscheck(self, group, new_tokens=24):
        """-> None if the p2p decode produced the same tokens on every rank with a clean error word, else the reason; the same
        verdict on every rank (one object all-gather reached by all)."""
        import torch.distributed as dist
        from usdm_amd.p2p import agree
        fail, toks = None, None
        try:
            ids = torch.randint(32002, 42002, (1, 96), generator=torch.Generator().manual_seed(7)).to(self.dev)
            toks = self.llm.generate(input_ids=ids, max_new_tokens=new_tokens)[0, 96:].tolist()
            err, _ = self.llm.p2p.status()
            if err:
                fail = f"error word {err:#x} after {new_tokens} tokens"
        except Exception as e:  # noqa: BLE001 - recorded; the agreement below is still reached
            fail = repr(e)
        world = dist.get_world_size(group)
        got = [None] * world
        dist.all_gather_object(got, toks, group=group)
        if fail is None and any(t != got[0] for t in got):
            fail = "token streams differ between ranks"
        self.llm._kv_ids = None
        return agree(group, fail)

    def _mark(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.setdefault(name, []).append(e)

    def step(self):
        a, dev = self.args, self.dev
        self.ev = {}
        self.llm._kv_ids = None       # utterances are independent: nothing cached by the previous step may be reused
        self._mark("t0")
        units = self.ue.predict(self.wave, 34)                                        # [499]
        self._mark("tok")
        unit_tok = units + 32002
        corr = torch.tensor([32001], device=dev)
        p1 = torch.cat([self.template_ids.to(dev), unit_tok, corr])[None]
        o1 = self.llm.generate(input_ids=p1, max_new_tokens=a.text_tokens, do_sample=True, top_k=1, top_p=1.0, temperature=1.0,
                               bad_words_ids=self.bad_u2t, eos_token_id=None)
        self._mark("llm1")
        p2 = torch.cat([o1[0], self.sep_ids.to(dev)])[None]
        o2 = self.llm.generate(input_ids=p2, max_new_tokens=a.text_tokens, do_sample=True, top_k=1, top_p=1.0, temperature=1.0,
                               bad_words_ids=self.bad_t2t, eos_token_id=None)
        self._mark("llm2")
        p3 = torch.cat([o2[0], corr])[None]
        o3 = self.llm.generate(input_ids=p3, max_new_tokens=a.units, do_sample=True, top_k=1, top_p=1.0, temperature=1.0,
                               bad_words_ids=self.bad_t2u, eos_token_id=None)
        self._mark("llm3")
        agent_units = (o3[0, p3.shape[1]:] - 32002).clamp_(0, 9999)
        audio = self.mu.reconstruct_speech(agent_units, dev, None, self.ue, self.vb, self.voc, n_timesteps=a.nt,
                                           reference_mel=self.ref_mel, reference_unit=self.ref_units, noise=self.noise,
                                           cfg_group=self.cfg_group)
        self._mark("dec")
        self.prompt_lens = (p1.shape[1], p2.shape[1], p3.shape[1])
        self.n_generated = 2 * a.text_tokens + a.units
        # what a caller of the path receives (references only: nothing is copied inside the timed step)
        self.outputs = {"units": units, "llm_asr_tokens": o1[0, p1.shape[1]:], "llm_t2t_tokens": o2[0, p2.shape[1]:],
                        "llm_tts_tokens": o3[0, p3.shape[1]:], "audio": audio}
        return audio

    def dump_outputs(self, d):
        """The last step's outputs as d/<name>.npy: audio in float32 (as returned), token ids in float64 (exact)."""
        import numpy as np
        os.makedirs(d, exist_ok=True)
        for name, v in self.outputs.items():
            v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            np.save(os.path.join(d, name + ".npy"), v.astype(np.float32 if v.dtype == np.float32 else np.float64))

    def stage_ms(self):
        torch.cuda.synchronize()
        g = lambda a, b: self.ev[a][0].elapsed_time(self.ev[b][0])
        return {"tokenizer": g("t0", "tok"), "llm_asr": g("tok", "llm1"), "llm_t2t": g("llm1", "llm2"), "llm_tts": g("llm2", "llm3"),
                "voicebox_vocoder": g("llm3", "dec")}


def gemv_rows(llm, a):
    """Rows a usdm_gemv launch has to stream: all of them, except in lm_head mode where rows whose id is banned are skipped."""
    if a.part_val and a.ban:
        return int((llm.ban == 0).sum().item())
    return a.N


def measure_gemv_roofline(llm):
    """Eager pass over one decode step with a HIP-event pair around every usdm_gemv launch (same stream)."""
    from usdm_amd import ops
    segs = llm._build_decode()
    stream = ops._stream()
    pairs, nbytes = [], 0
    for rep in range(3):
        pairs, nbytes = [], 0
        for s in segs:
            if not isinstance(s, ops.Plan):
                s()
                continue
            for what, fn, args in s.calls:
                if what == "usdm_gemv":
                    a = args[0]._obj
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(*args, stream)
                    e1.record()
                    pairs.append((e0, e1))
                    nbytes += 2 * gemv_rows(llm, a) * a.K
                else:
                    fn(*args, stream)
        torch.cuda.synchronize()
    ms_step = sum(e0.elapsed_time(e1) for e0, e1 in pairs)
    n = len(pairs)
    ach_step = nbytes / (ms_step * 1e-3) / 1e9
    # Kernel-only duration: the launches of each shape (one per layer, each over its own cold weights) replayed back to back as
    # a hipGraph between ONE event pair, so that neither the host nor the per-launch event packets sit between kernels.  This is
    # the average launch duration that the rocprofv3 kernel stats in profiles/ report; the per-launch pairs above additionally
    # contain the event packets and launch gaps of an eager step.
    ms, groups = ms_step, None
    if llm.tp_size == 1 and not llm.tp_path:
        from usdm_amd.graph import GraphedPlan
        by = {}
        for s_ in segs:
            if isinstance(s_, ops.Plan):
                for what, fn, args in s_.calls:
                    if what == "usdm_gemv":
                        a = args[0]._obj
                        by.setdefault((a.N, a.K, a.act), []).append((what, fn, args))
        ms, groups = 0.0, {}
        for key, calls in by.items():
            sub = ops.Plan()
            sub.calls = calls
            gp = GraphedPlan(sub)
            for _ in range(3):
                gp.run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                gp.run()
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) / 3
            ms += t
            groups[f"N{key[0]}xK{key[1]}" + ("(swiglu)" if key[2] == 3 else "")] = round(t * 1e3 / len(calls), 2)
    ach = nbytes / (ms * 1e-3) / 1e9
    # the o_proj launch of the shipped step carries the attention merge (usdm_gemv cmb_gran, llm.cmb): its kernel-only duration is
    # part of `achieved` above as it ships; the same launch WITHOUT the merge (separate combine kernel) is timed beside it
    oproj_plain_us = None
    if groups is not None and llm.cmb:
        from usdm_amd.graph import GraphedPlan
        llm.cmb = False
        try:
            calls = [c for s_ in llm._build_decode() if isinstance(s_, ops.Plan) for c in s_.calls
                     if c[0] == "usdm_gemv" and c[2][0]._obj.N == 4096 and c[2][0]._obj.K == 4096]
        finally:
            llm.cmb = True
        sub = ops.Plan()
        sub.calls = calls
        gp = GraphedPlan(sub)
        for _ in range(3):
            gp.run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            gp.run()
        e1.record()
        torch.cuda.synchronize()
        oproj_plain_us = round(e0.elapsed_time(e1) / 3 * 1e3 / len(calls), 2)
    traffic, traffic_src = None, None
    try:  # PMC counters cannot be read from inside this process: use the committed rocprofv3 --pmc record of the same kernel, and
        # only if it was measured on the kernel source that is compiled now (tools/r04_profile.sh stores its sha256)
        import hashlib
        rec = json.load(open(os.path.join(ROOT, "profiles", "r04_gemv_pmc.json")))
        sha = hashlib.sha256(open(os.path.join(ROOT, "usdm_amd", "csrc", "llm_k.hip"), "rb").read()).hexdigest()
        if llm.tp_size == 1:
            if rec.get("llm_k_hip_sha256") == sha:
                traffic, traffic_src = rec["hbm_bytes_per_launch"], rec["source"]
            else:
                traffic_src = "profiles/r04_gemv_pmc.json is stale (measured on another llm_k.hip): traffic withheld"
    except Exception:
        pass
    return {"bound": "hbm", "kernel": "gemv_kernel (usdm_gemv, 7B decode weight streaming)", "achieved": round(ach, 1),
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
            "launches_per_token": n, "avg_launch_us": round(ms * 1e3 / n, 2), "avg_bytes_per_launch": int(nbytes / n),
            "algorithmic_bytes_per_token": int(nbytes), "avg_launch_us_by_shape": groups,
            "attention_merge": ("inside the o_proj launch (usdm_gemv cmb_gran): its duration is counted as shipped" if llm.cmb else "separate combine kernel"),
            "o_proj_launch_us_without_merge": oproj_plain_us,
            "achieved_in_eager_step": round(ach_step, 1), "avg_launch_us_in_eager_step": round(ms_step * 1e3 / n, 2),
            "method": "achieved: each GEMV shape's per-layer launches replayed back to back (hipGraph) between one HIP event pair; "
                      "achieved_in_eager_step: event pair around every launch of an eager decode step (adds event packets and launch gaps)"}


def host_cores():
    """Threads the CPU baseline may use: the cgroup CPU quota if one is set, else the affinity mask,
    capped at 16 (the CPU share of a one-GPU box; more threads only oversubscribe it)."""
    n = None
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, int(int(q) / int(p)))
    except Exception:
        pass
    if n is None:
        try:
            n = len(os.sched_getaffinity(0))
        except Exception:
            n = os.cpu_count() or 1
    return max(1, min(n, 16))


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(args, dev, pipe):
    """CPU oracle (kind 'port') on the host cores, as BASELINE.md section 4 states it: the FULL-size models (weights generated on the
    GPU and copied to the host), tokenizer and BigVGAN timed in full, the 7B over a 128-token prefill + 16 decode tokens and the
    Voicebox over 3 CFG-doubled NFEs, each scaled to the workload of one bench step.  About 30 s of CPU work."""
    from oracle import bigvgan_oracle as BO, mistral_oracle as MO, voicebox_oracle as VO, w2v_oracle as WO
    from usdm_amd import synth
    cores = host_cores()
    torch.set_num_threads(cores)
    out = {}
    nfe = 2 * ((args.nt + 1) // 2) - 1
    frames = (args.units * 441) // 256
    with torch.no_grad():
        # tokenizer, in full: 10 s of audio through all 35 layers + 10 000-centroid k-means
        cfg = dict(WO.XLSR_1B)
        sd = {k: v.cpu() for k, v in synth.w2v_state_dict(dev).items()}
        cen = synth.w2v_centroids(dev).cpu()
        wave = pipe.wave.detach().cpu()                   # the step's own input (identical inputs)
        t = time.time(); WO.kmeans_assign(WO.features(sd, cfg, wave, 34), cen); out["tokenizer_s"] = time.time() - t
        del sd, cen
        # BigVGAN, in full: 861 frames
        h = dict(BO.BIGVGAN_22K_80)
        sd = BO.random_state_dict(h, 0)
        mel = torch.randn(1, 80, frames, generator=torch.Generator().manual_seed(1)) * 2.1575 - 5.5419
        t = time.time(); BO.bigvgan_forward(sd, h, mel); out["bigvgan_s"] = time.time() - t
        del sd
        # Voicebox: 3 CFG-doubled NFEs at full depth and length (S = 256 + frames), scaled to the step's NFE count
        cfg = dict(VO.VOICEBOX_CFG)
        sd = VO.random_state_dict(cfg, 0)
        S = 256 + frames
        x = torch.randint(0, 10000, (2, S)); y = torch.randn(2, 80, S)
        t = time.time()
        for _ in range(3):
            VO.estimator_forward(sd, cfg, x, y, y, torch.full((2, 1, 1), 0.5), torch.tensor([S, S]))
        out["voicebox_s"] = (time.time() - t) / 3 * nfe
        del sd
        # 7B, all 32 layers, bf16: 128-token prefill (scaled to the three prompts) + 16 decode tokens (scaled to the generated count)
        cfg = dict(MO.MISTRAL_7B_USDM)
        sd = {k: v.cpu() for k, v in synth.random_llm_state_dict(cfg, dev, seed=3).items()}
        torch.cuda.empty_cache()
        ids = torch.randint(32002, 42002, (128,))
        t = time.time(); _, cache = MO.forward(sd, cfg, ids); tp = time.time() - t
        t = time.time()
        for _ in range(16):
            _, cache = MO.forward(sd, cfg, ids[:1], cache)
        td = (time.time() - t) / 16
        prompt_tokens = int(sum(pipe.prompt_lens))       # the three prompts of the timed step (the reference re-prefills each round)
        n_gen = 2 * args.text_tokens + args.units
        out["llm_s"] = tp * prompt_tokens / 128 + td * n_gen
        out_tok = 1.0 / td
        del sd, cache
    total = sum(out.values())
    return {"value": round(9.996 / total, 5), "unit": "x real-time", "cores": cores, "cpu": cpu_model(), "kind": "port",
            "stage_seconds": {k: round(v, 2) for k, v in out.items()},
            "llm_decode_tokens_per_s": round(out_tok, 3), "llm_tokens_per_s": round(n_gen / out["llm_s"], 3),
            "sample": f"CPU oracle (oracle/*.py, torch CPU, {cores} threads), full-size models: XLS-R tokenizer in full (10 s, 35 layers, "
                      f"k-means); BigVGAN in full ({frames} frames); Voicebox 3 CFG-doubled NFEs at full depth, S={256 + frames} "
                      f"(x{nfe}/3); Mistral-7B all 32 layers bf16: 128-token prefill (x{prompt_tokens}/128) + 16 decode tokens (x{n_gen}/16)"}


def batched_decode_rate(llm, B=4, new_tokens=96):
    """Informational (outside the timed region): aggregate decode tokens/s of generate_batch — B utterances in lockstep, weights
    streamed once per step (B <= 4: VALU kernel, above: the matrix-core form of usdm_gemv_batch).  Not part of `value`."""
    dev = llm.device
    gen = torch.Generator().manual_seed(11)
    prompts = [torch.randint(32002, 42002, (1, 560 - 8 * b), generator=gen).to(dev) for b in range(B)]
    llm.generate_batch(prompts, max_new_tokens=24)      # plans + graph capture
    torch.cuda.synchronize()
    t = time.perf_counter(); llm.generate_batch(prompts, max_new_tokens=8); torch.cuda.synchronize(); t1 = time.perf_counter() - t
    t = time.perf_counter(); llm.generate_batch(prompts, max_new_tokens=8 + new_tokens); torch.cuda.synchronize(); t2 = time.perf_counter() - t
    ms = 1e3 * (t2 - t1) / new_tokens
    wb = llm.weight_bytes_per_token()
    return {"batch": B, "tokens_per_s": round(B * new_tokens / (t2 - t1), 1), "ms_per_step": round(ms, 3),
            "weight_stream_gbs": round(wb / (ms * 1e-3) / 1e9, 1), "frac_of_hbm_spec": round(wb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 3),
            "kernel": "gemv_batch_kernel (VALU)" if B <= 4 else "gemv_mfma_kernel (v_mfma_f32_16x16x32_bf16, weights as the A operand)",
            "note": "aggregate over the batch; decode steps only (whole step incl. attention over B caches and the token pick)"}


def pipeline_throughput(pipe, N=16, vb_batch=4):
    """Informational (outside the timed region, never `value`): N utterances through all four stages, batched where the stage
    batches - the tokenizer per utterance, the 7B's three rounds as ONE batched decode of N sequences (generate_batch, matrix-core
    form), the Voicebox solve at batch vb_batch (x 2 for CFG), BigVGAN per utterance - aggregate output audio seconds per wall
    second.  What the serving path's request lists buy (src/inference_vllm.py:109-125; src/streamlit_demo.py:258-287)."""
    a, dev, llm = pipe.args, pipe.dev, pipe.llm
    mu = pipe.mu

    def run():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        t0 = time.perf_counter()
        units = [pipe.ue.predict(pipe.wave, 34) for _ in range(N)]
        ev[0].record()
        corr = torch.tensor([32001], device=dev)
        p1 = [torch.cat([pipe.template_ids.to(dev), u + 32002, corr])[None] for u in units]
        o1 = llm.generate_batch(p1, max_new_tokens=a.text_tokens, bad_words_ids=pipe.bad_u2t)
        p2 = [torch.cat([o[0], pipe.sep_ids.to(dev)])[None] for o in o1]
        o2 = llm.generate_batch(p2, max_new_tokens=a.text_tokens, bad_words_ids=pipe.bad_t2t)
        p3 = [torch.cat([o[0], corr])[None] for o in o2]
        o3 = llm.generate_batch(p3, max_new_tokens=a.units, bad_words_ids=pipe.bad_t2u)
        ev[1].record()
        hps = pipe.voc.h
        agent = [mu.process_unit((o[0, p.shape[1]:] - 32002).clamp_(0, 9999), hps, dev)[0] for o, p in zip(o3, p3)]     # [1, frames] each
        ref_u, _ = mu.process_unit(pipe.ref_units, hps, dev)
        P = ref_u.shape[-1]
        ref_mel = (pipe.ref_mel[:, :, :P] - mu.mel_mean) / mu.mel_std
        mels = []
        for g0 in range(0, N, vb_batch):
            grp = agent[g0:g0 + vb_batch]
            B = len(grp)
            unit = torch.cat([torch.cat([ref_u, u], -1) for u in grp], 0)
            S = unit.shape[-1]
            y = torch.zeros(B, hps.num_mels, S, device=dev)
            y[:, :, :P] = ref_mel
            y_dec = pipe.vb.generate(unit, y, torch.full((B,), S, dtype=torch.long, device=dev), n_timesteps=a.nt, solver="heun",
                                     gradient_scale=1.0, speech_prompt=True, prompt_lengths=torch.full((B,), P, dtype=torch.long, device=dev),
                                     noise=pipe.noise.expand(-1, B, -1, -1).contiguous())
            mels.append(y_dec[:, :, P:])
        ev[2].record()
        audio = [pipe.voc.forward(m[b:b + 1].contiguous(), mu.mel_std, mu.mel_mean) for m in mels for b in range(m.shape[0])]
        ev[3].record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        n_samples = sum(int(x.numel()) for x in audio)
        return wall, n_samples, ev

    run()                                                    # plans, graphs
    wall, n_samples, ev = run()
    audio_s = n_samples / 22050.0
    st = {"llm_3_rounds_batched": ev[0].elapsed_time(ev[1]) * 1e-3, "voicebox": ev[1].elapsed_time(ev[2]) * 1e-3, "bigvgan": ev[2].elapsed_time(ev[3]) * 1e-3}
    st["tokenizer"] = wall - sum(st.values())
    return {"utterances": N, "audio_s": round(audio_s, 2), "wall_s": round(wall, 3), "value": round(audio_s / wall, 2),
            "unit": "x real-time, aggregate over the utterances", "llm_batch": N, "voicebox_batch": f"{vb_batch} utterances x 2 (CFG)",
            "stage_s": {k: round(v, 3) for k, v in st.items()},
            "note": "informational; the headline `value` stays the single utterance"}


def self_launch(args):
    """`python bench.py --gpus N` typed directly (no RANK in the environment): this process has made NO GPU call yet (importing
    torch does not initialise HIP), so it starts the N ranks as fresh child processes through torch.distributed.run, lets them
    inherit stdout (rank 0 prints the JSON line) and exits with the launcher's code.  Never an exec of a GPU-holding process."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def launch_check(rank, world):
    """USDM_BENCH_LAUNCH_CHECK=1 (CPU test of the launch plumbing, tests/test_bench_launch_cpu.py): rendezvous over gloo, barrier,
    rank 0 prints one JSON line.  No GPU, no model."""
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.ones(1)
    dist.all_reduce(t)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"launch_check": True, "world": world, "sum": int(t.item())}), flush=True)
    dist.destroy_process_group()


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(args))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if os.environ.get("USDM_BENCH_LAUNCH_CHECK") == "1":
        return launch_check(rank, world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    # USDM_BENCH_SHARE_GPU=1 (validation of the multi-rank path on a box with fewer GPUs than ranks): ranks share devices, the
    # process group is gloo (RCCL refuses two ranks on one device; the prefill collectives are then staged through the host) and
    # the decode exchange is the peer-to-peer one over hipIpc.  Numbers from such a run are not scaling results.
    share = os.environ.get("USDM_BENCH_SHARE_GPU") == "1"
    ndev = torch.cuda.device_count()
    if world > ndev and not share:
        raise SystemExit(f"bench.py: {world} ranks but {ndev} GPU(s) (USDM_BENCH_SHARE_GPU=1 lets ranks share a device for validation)")
    local = local % ndev
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    group = None
    dist_on = world > 1 or args.force_dist
    if dist_on:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if share and world > ndev:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        group = dist.group.WORLD

    def barrier():
        if dist_on:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    pipe = Pipeline(dev, rank, world, group, args)
    for _ in range(args.warmup):
        audio = pipe.step()
    barrier()
    t0 = time.perf_counter()
    stage_acc = None
    for _ in range(args.steps):
        audio = pipe.step()
        if stage_acc is None:
            stage_acc = pipe.ev
    barrier()
    dt = time.perf_counter() - t0
    if dist_on:
        import torch.distributed as dist
        host = dist.get_backend() == "gloo"
        t = torch.tensor([dt], device="cpu" if host else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    stages = pipe.stage_ms()  # last step
    audio_s = audio.shape[0] / 22050.0
    ms_per_step = dt * 1e3 / args.steps
    llm_ms = stages["llm_asr"] + stages["llm_t2t"] + stages["llm_tts"]
    res = {
        "metric": METRIC, "value": round(audio_s * args.steps / dt, 4), "unit": "x real-time (output audio s / wall s)",
        "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 2),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "bf16", "dtype_detail": "LLM + Voicebox: bf16 MFMA operands, f32 accumulate; tokenizer + vocoder: exact f32 MFMA"
                 if args.vocoder_dtype == "f32" else "LLM + Voicebox + vocoder convs bf16 MFMA; tokenizer f32",
        "data": "synthetic",
        "config": {"workload": "full pipeline, one 10 s utterance: XLS-R tokenizer -> Mistral-7B (3 greedy rounds) -> "
                               "Token-Voicebox 63 NFE (Heun, CFG, 3 s prompt) -> BigVGAN",
                   "wave_samples": 160000, "prompt_tokens": list(pipe.prompt_lens), "generated_tokens": pipe.n_generated,
                   "voicebox_n_timesteps": args.nt, "mel_frames": pipe.frames, "output_samples": int(audio.shape[0]),
                   "reference_front_end": "outside the timed region (inputs per SURVEY 8d: reference_mel / reference_unit handed over; "
                                          "sample(--reference_path) would add the prompt's tokenizer pass + get_mel, ~15-20 ms)",
                   "parallelism": f"tp{world} (LLM) + replicas", "tp_comm": pipe.tp_comm, "voicebox": pipe.vb_mode,
                   **({"shared_gpu_validation": f"{world} ranks on {torch.cuda.device_count()} GPU(s): code-path validation, not a scaling result"}
                      if os.environ.get("USDM_BENCH_SHARE_GPU") == "1" and world > torch.cuda.device_count() else {})},
        "llm_tokens_per_s": round(pipe.n_generated / (llm_ms * 1e-3), 2),
        "llm_decode_tokens_per_s_tts_round": round(args.units / (stages["llm_tts"] * 1e-3), 2),
        "stage_ms": {k: round(v, 2) for k, v in stages.items()},
        "model_build_s": round(pipe.build_s, 1),
    }
    if args.dump_outputs and rank == 0:
        pipe.dump_outputs(args.dump_outputs)
    if args.full:
        full_measurements(args, pipe, res, stages, dev, rank, world, dist_on)
    if dist_on:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(res), flush=True)


def full_measurements(args, pipe, res, stages, dev, rank, world, dist_on):
    """--full: everything beside the headline figures, each measured in runs of its own after the timed steps."""
    # secondary rooflines (informational): MFMA-bound stages, algorithmic FLOPs from SURVEY.md §8d
    mel = torch.randn(1, 80, pipe.frames, device=dev) * 2.1575 - 5.5419
    pipe.voc(mel)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    pipe.voc(mel)
    e1.record()
    torch.cuda.synchronize()
    voc_ms = e0.elapsed_time(e1)
    vb_ms = max(stages["voicebox_vocoder"] - voc_ms, 1e-3)
    nfe = 2 * ((args.nt + 1) // 2) - 1
    res["stage_rooflines"] = {
        "voicebox": {"bound": "mfma", "dtype": "bf16", "tflop": round(1.734 * nfe, 1), "ms": round(vb_ms, 1),
                     "achieved_tflops": round(1.734 * nfe / (vb_ms * 1e-3), 1), "peak_tflops": 2500.0},
        "bigvgan": {"bound": "mfma", "dtype": "f32", "tflop": round(1.833e-3 * pipe.frames, 3), "ms": round(voc_ms, 2),
                    "achieved_tflops": round(1.833e-3 * pipe.frames / (voc_ms * 1e-3), 1), "peak_tflops": 157.3},
        "tokenizer": {"bound": "mfma", "dtype": "f32", "tflop": 0.80, "ms": round(stages["tokenizer"], 2),
                      "achieved_tflops": round(0.80 / (stages["tokenizer"] * 1e-3), 1), "peak_tflops": 157.3},
    }
    if rank == 0:
        res["roofline"] = measure_gemv_roofline(pipe.llm)
        if world == 1 and not dist_on and not args.no_batched:
            res["llm_batched_decode"] = []
            for B in (4, 8, 16):
                try:
                    res["llm_batched_decode"].append(batched_decode_rate(pipe.llm, B))
                except Exception as e:  # noqa: BLE001 - informational field only, must never break the bench line
                    res["llm_batched_decode"].append({"batch": B, "error": repr(e)})
            try:
                res["pipeline_throughput"] = pipeline_throughput(pipe)
            except Exception as e:  # noqa: BLE001
                res["pipeline_throughput"] = {"error": repr(e)}
        if world == 1 and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(args, dev, pipe)
    elif dist_on:
        measure_gemv_roofline(pipe.llm)  # collectives inside the TP decode need every rank


if __name__ == "__main__":
    main()
