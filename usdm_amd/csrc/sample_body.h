// The draw of the sampling kernels (sample_k.hip), included as text into sample_final_kernel<SEG> (the pick of a decode step) and
// spec_sample_kernel (the T rows of a sampled speculative step): sanitise the knobs, temperature -> top-k -> top-p -> min-p -> one
// Philox draw, the fallback where no id has mass.  Expects `a` (usdm_sample_args whose logits point at THIS row), `st` (its step
// words), b (the sequence: dev_params[b], step[b]), row_i (the Philox counter is step[b] + row_i; the decode step's is the constant
// 0), tid, V, SEG and seg_stride / seg_len / seg_magic; leaves s_tok (the local id, after a barrier), Zk, pkey, El, Q, each and
// step.  Text and not a device function so that both sample_final_kernel instantiations compile to the code they had before the
// speculative kernel existed (profiles/spec_sample_isa_diff.txt).
  __shared__ unsigned long long hist[256];
  __shared__ unsigned long long sscan[NT];
  __shared__ float sred[NT / 64];
  __shared__ unsigned s_prefix;
  __shared__ unsigned long long s_rem;
  __shared__ int s_tok;
  if (a.dev_params) {   // per-request knobs live in device memory: one captured graph for every request
    a.dev_params += b;
    a.temperature = a.dev_params->temperature; a.top_k = a.dev_params->top_k; a.top_p = a.dev_params->top_p; a.seed = a.dev_params->seed;
    if (!(a.temperature > 0.f)) a.temperature = 1.0f;
    if (!(a.top_p > 0.f) || a.top_p > 1.0f) a.top_p = 1.0f;
    if (a.top_k < 0) a.top_k = 0;
    a.min_p = (a.dev_params->min_p >= 0.f && a.dev_params->min_p <= 1.0f) ? a.dev_params->min_p : 0.f;   // (NaN fails both)
  }
  const float invT = 1.0f / a.temperature;   // HF divides; x / T and x * (1 / T) differ by <= 1 ulp, below the logits' bf16 grain
  // the scaled logit as every stage sees it.  -0.0 becomes +0.0: HF's `scores < kth` compares values, to which the two zeros are
  // equal, while fkey orders -0.0 one key below +0.0 and would drop the -0.0 entries of a zero tie block at the k-th rank
  auto SC = [&](float lg) -> float { const float x = lg * invT; return x == 0.f ? 0.f : x; };
  const logits_row_view rv{seg_stride, seg_len, seg_magic};
  auto LG = [&](int i) -> float { return row_at<SEG>(a.logits, i, rv); };
  auto each = [&](auto&& f) {   // f(i, logit of i) for i = tid, tid + NT, ... < V
    row_each<SEG, NT>(a.logits, V, tid, rv, [&](int i, const float* px) { f(i, *px); });
  };

  // ---- top-k: key of the k-th largest scaled logit (all keys >= it are kept, ties included: `scores < kth` is removed)
  unsigned kth = 0;   // keep everything
  if (a.top_k > 0 && a.top_k < V) {
    unsigned prefix = 0, mask = 0;
    unsigned long long rem = (unsigned long long)a.top_k;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      each([&](int, float lg) {
        const unsigned k = fkey(SC(lg));
        if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1ull);
      });
      __syncthreads();
      if (tid == 0) {
        unsigned long long r = rem;
        int b = 255;
        for (; b > 0; --b) {
          if (hist[b] >= r) break;
          r -= hist[b];
        }
        s_prefix = prefix | ((unsigned)b << shift);
        s_rem = r;
      }
      __syncthreads();
      prefix = s_prefix; rem = s_rem; mask |= 255u << shift;
      __syncthreads();
    }
    kth = prefix;
  }
  // ---- softmax numerators over the top-k survivors
  float m = -INFINITY;
  each([&](int, float lg) {
    const float x = SC(lg);
    if (fkey(x) >= kth) m = fmaxf(m, x);
  });
  m = block_max(m, sred);
  auto El = [&](float lg) -> float {   // exp(x - max) of a top-k survivor, 0 otherwise (banned = -inf -> 0)
    const float x = SC(lg);
    return (fkey(x) >= kth) ? __expf(x - m) : 0.f;
  };
  auto Ei = [&](int i) -> float { return El(LG(i)); };
  auto Q = [&](float e) -> unsigned long long { return (unsigned long long)((double)e * 4294967296.0); };   // 2^32 fixed point
  // total mass (fixed point, integer sum: order-independent)
  if (tid == 0) s_rem = 0;
  __syncthreads();
  {
    unsigned long long z = 0;
    each([&](int, float lg) { z += Q(El(lg)); });
    atomicAdd(&s_rem, z);
  }
  __syncthreads();
  const unsigned long long Ztot = s_rem;
  __syncthreads();
  // ---- top-p: drop the ascending tail whose cumulative mass stays <= (1 - top_p) * Z
  unsigned pkey = 0;   // keep e-keys >= pkey (keys of positive floats are ordered like the floats)
  if (a.top_p < 1.0f) {
    unsigned long long R = (unsigned long long)((1.0 - (double)a.top_p) * (double)Ztot);
    unsigned prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      each([&](int, float lg) {
        const float e = El(lg);
        if (e > 0.f) {
          const unsigned k = __float_as_uint(e);
          if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255], Q(e));
        }
      });
      __syncthreads();
      if (tid == 0) {
        unsigned long long r = R;
        int b = 0;
        for (; b < 255; ++b) {
          if (hist[b] > r) break;      // including bin b would exceed the removable mass: the threshold is inside it
          r -= hist[b];
        }
        s_prefix = prefix | ((unsigned)b << shift);
        s_rem = r;
      }
      __syncthreads();
      prefix = s_prefix; R = s_rem; mask |= 255u << shift;
      __syncthreads();
    }
    pkey = prefix;
  }
  // ---- min-p: drop e_i < min_p (e_i = p_i / p_max; the maximum has e = 1 and survives top-k and top-p, so the kept set is the
  // intersection).  Keys of positive floats are ordered like the floats, so the f32 test e >= min_p is one more bound on the key
  if (a.min_p > 0.f) pkey = max(pkey, __float_as_uint(a.min_p));
  // ---- draw: contiguous index ranges, exclusive scan of the kept fixed-point masses
  const int per = (V + NT - 1) / NT;
  const int i0 = tid * per, i1 = min(V, i0 + per);
  unsigned long long loc = 0;
  for (int i = i0; i < i1; ++i) {
    const float e = Ei(i);
    if (e > 0.f && __float_as_uint(e) >= pkey) loc += Q(e);
  }
  sscan[tid] = loc;
  __syncthreads();
  for (int off = 1; off < NT; off <<= 1) {   // Hillis-Steele inclusive scan
    const unsigned long long v = tid >= off ? sscan[tid - off] : 0ull;
    __syncthreads();
    sscan[tid] += v;
    __syncthreads();
  }
  const unsigned long long Zk = sscan[NT - 1];
  const int step = st.step[b] + row_i;
  // top_k == 1 is the reference's "greedy" (do_sample=True, top_k=1): among exact ties take the lowest id, as usdm_argmax_final does
  const double u = a.top_k == 1 ? 0.0 : philox_uniform(a.seed, (unsigned)step);
  unsigned long long target = (unsigned long long)(u * (double)Zk);
  if (Zk > 0 && target >= Zk) target = Zk - 1;
  const unsigned long long excl = sscan[tid] - loc;
  if (tid == 0) s_tok = -1;
  __syncthreads();
  if (loc > 0 && excl <= target && target < excl + loc) {
    unsigned long long c = excl;
    int pick = i0;
    for (int i = i0; i < i1; ++i) {
      const float e = Ei(i);
      if (e > 0.f && __float_as_uint(e) >= pkey) {
        const unsigned long long q = Q(e);
        if (target < c + q) { pick = i; break; }
        c += q;
      }
    }
    s_tok = pick;
  }
  __syncthreads();
  if (s_tok < 0) {   // no id has positive mass (all banned / NaN logits): arg-max of the finite logits, else id 0
    __shared__ float fbv[NT / 64];
    __shared__ int fbi[NT / 64];
    float bv = -INFINITY;
    int bi = PICK_NO_ID;
    each([&](int i, float x) {
      if (x > bv) { bv = x; bi = i; }     // NaN and -inf never pass
    });
    pick_wave_best(bv, bi);
    if ((tid & 63) == 0) { fbv[tid >> 6] = bv; fbi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < NT / 64; ++w)
        if (pick_better(fbv[w], fbi[w], bv, bi)) { bv = fbv[w]; bi = fbi[w]; }
      s_tok = bi == PICK_NO_ID ? 0 : bi;
    }
    __syncthreads();
  }
