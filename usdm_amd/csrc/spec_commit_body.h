// The body of the speculative commit kernels (spec_k.hip), included as text into spec_commit_kernel (one sequence) and
// spec_commit_batch_kernel (one workgroup per slot): expects `a` (usdm_spec_args) and `st` (usdm_decode_state) of ONE sequence, the
// embedding table E, Hd and that sequence's h_out rows.  Text and not a device function so that the single-sequence kernel compiles
// to the code it had before the batch kernel existed (profiles/spec_batch_isa_diff.txt).  SPEC_GIVEN_PICKS defined around the
// include (the *_picks kernels): the pick stage reads `picks`, this sequence's T local ids, instead of arg-maxing
// the partials; everything behind it is the same text.
  __shared__ float sv[256];
  __shared__ int si[256];
  __shared__ int s_g[SP_TMAX], s_d[SP_TMAX];
  __shared__ int s_step, s_next, s_stop;
  const int tid = threadIdx.x, T = a.T;
  if (st.done && st.done[0]) return;
  if (!a.propose_only) {
#ifdef SPEC_GIVEN_PICKS
    // ---- picks: given as local ids (usdm_spec_sample's draws), `picks` of this sequence's T rows
    if (tid < T) s_g[tid] = picks[tid] + st.id_offset;
    __syncthreads();
#else
    // ---- picks: row i's arg-max over its partials, usdm_argmax_final's reduction
    for (int i = 0; i < T; ++i) {
      const float* pv = a.part_val + (int64_t)i * a.nparts;
      const int* pi = a.part_idx + (int64_t)i * a.nparts;
      float bv = -INFINITY;
      int bi = PICK_NO_ID;
      for (int k = tid; k < a.nparts; k += 256) {
        const float v = pv[k];
        const int id = pi[k];
        if (pick_better(v, id, bv, bi)) { bv = v; bi = id; }
      }
      pick_block_best<256>(sv, si, bv, bi);
      if (tid == 0) s_g[i] = (si[0] == PICK_NO_ID ? 0 : si[0]) + st.id_offset;
      __syncthreads();
    }
#endif
    // ---- accept and commit (one thread: at most 8 tokens)
    if (tid == 0) {
      const int s0 = st.step[0];
      const int lim = min(*a.limit, st.max_out);
      int stop = 0;
      if (s0 >= lim) {
        if (st.done) st.done[0] = 1;
        stop = 1;
      } else {
        int n = 0, drafted = 0;
        while (n < T - 1 && a.drafts[n + 1] == s_g[n]) ++n;
        for (int i = 1; i < T; ++i) drafted += a.drafts[i] >= 0;
        const int neos = st.eos ? min(st.eos[0], 6) : 0, mn = st.eos ? st.eos[1] : 0;
        int m = 0, done = 0;
        for (int i = 0; i <= n && s0 + m < lim; ++i) {
          const int tok = s_g[i];
          st.out_tokens[s0 + m] = tok;
          ++m;
          bool hit = false;
          for (int e = 0; e < neos; ++e) hit |= (st.eos[2 + e] == tok);
          if (hit && s0 + m >= mn) { done = 1; break; }
        }
        if (s0 + m >= lim) done = 1;
        st.step[0] = s0 + m;
        st.pos[0] = st.pos[0] + m;
        st.next_token[0] = st.out_tokens[s0 + m - 1];
        if (done && st.done) st.done[0] = 1;
        a.counters[0] += 1;
        a.counters[1] += drafted;
        a.counters[2] += m - 1;
      }
      s_stop = stop;
    }
    __syncthreads();
    if (s_stop) return;
  }
  if (tid == 0) { s_step = st.step[0]; s_next = st.next_token[0]; }
  if (tid < SP_TMAX) s_d[tid] = -1;
  __syncthreads();
  // ---- propose the next step's drafts
  const int step = min(max(s_step, 0), st.max_out);
  const int P = min(max(*a.prompt_len, 0), a.prompt_max);
  const int Lh = P + step;
  if (a.script && a.params[2]) {
    if (tid >= 1 && tid < T) {
      const int j = step + tid - 1;
      s_d[tid] = j < st.max_out ? a.script[j] : -1;
    }
  } else {
    const int nmax = min(a.params[0], SP_NMAX), nmin = max(a.params[1], 1);
    for (int n = nmax; n >= nmin; --n) {
      if (Lh < n + 1) continue;
      int best = -1;
      for (int j = tid; j <= Lh - n - 1; j += 256) {      // ascending: the thread's last match is its most recent
        bool eq = true;
        for (int e = 0; e < n && eq; ++e) eq = spec_hist(a, st, P, j + e) == spec_hist(a, st, P, Lh - n + e);
        if (eq) best = j;
      }
      si[tid] = best;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) si[tid] = max(si[tid], si[tid + s]);
        __syncthreads();
      }
      const int jb = si[0];
      __syncthreads();
      if (jb < 0) continue;
      if (tid >= 1 && tid < T) {
        const int j = jb + n + tid - 1;
        s_d[tid] = j < Lh ? spec_hist(a, st, P, j) : -1;
      }
      break;
    }
  }
  __syncthreads();
  if (tid >= 1 && tid < T) {
    int d = s_d[tid];
    if (d - st.id_offset < 0 || d - st.id_offset >= a.V) d = -1;
    s_d[tid] = d;
    a.drafts[tid] = d;
  }
  __syncthreads();
  // ---- the next step's input rows: the token to continue from, then the drafts (no draft: the row of id 0, its pick is ignored)
  for (int i = 0; i < T; ++i) {
    const int tok = i == 0 ? s_next : (s_d[i] >= 0 ? s_d[i] : st.id_offset);
    pick_embed_row<256>(E, tok, Hd, h_out + (int64_t)i * Hd);
  }
