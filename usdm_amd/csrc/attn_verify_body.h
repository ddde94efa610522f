// The body of the verify-attention kernels (llm_attn_k.hip), included as text into attn_verify_kernel<G, MB> (one sequence) and
// attn_verify_batch_kernel<G, MB> (slot blockIdx.z of B): expects `a`, a usdm_attn_verify_args of ONE sequence, G and MB.  Text and not
// a device function so that the single-sequence kernels compile to the code they had before the batch kernels existed
// (profiles/spec_batch_isa_diff.txt): inlined through a function the same statements were scheduled differently.
  constexpr int M = MB * 16;
  // scores [M][AV_SLD] f32; after the softmax the same bytes hold the V tile [AV_KT][AV_VLD] bf16
  __shared__ __attribute__((aligned(16))) char raw[M * AV_SLD * 4 > AV_KT * AV_VLD * 2 ? M * AV_SLD * 4 : AV_KT * AV_VLD * 2];
  __shared__ __attribute__((aligned(16))) bf16_t qb[M][AV_VLD];
  __shared__ __attribute__((aligned(16))) bf16_t kn[AV_TMAX][128], vn[AV_TMAX][128];
  __shared__ __attribute__((aligned(16))) bf16_t pb[M][AV_PLD];
  static_assert(AV_KT * AV_VLD * 2 <= (int)sizeof(raw), "the V tile fits the score bytes");
  float (*sc)[AV_SLD] = (float (*)[AV_SLD])raw;
  bf16_t (*vs)[AV_VLD] = (bf16_t (*)[AV_VLD])raw;
  if (a.skip && *a.skip) return;
  const int kh = blockIdx.x, sp = blockIdx.y, NSP = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lc = lane >> 4;
  const int pos = *a.pos;
  if ((unsigned)pos >= (unsigned)a.ctx_max) return;
  const int Tl = min(a.T, a.ctx_max - pos);      // rows at positions < ctx_max
  const int last = pos + Tl - 1;
  const int kbeg = sp * a.C;
  if (kbeg > last) return;                       // past the live context
  const int kend = min(kbeg + a.C, last + 1);    // keys [kbeg, kend)
  const int tb0 = max(kbeg, av_lo(pos, a.window) & ~(AV_KT - 1));   // first tile any row sees a key of
  const bf16_t* qkv = (const bf16_t*)a.qkv;
  const bf16_t* Kc = (const bf16_t*)a.kcache + (int64_t)kh * a.ctx_max * 128;
  const bf16_t* Vc = (const bf16_t*)a.vcache + (int64_t)kh * a.ctx_max * 128;
  // ---- rope of the Tl x G q rows and the Tl k rows, the v rows as they are; dead q rows are zero
  for (int it = tid; it < Tl * (G + 1) * 64; it += 256) {
    const int i = it / ((G + 1) * 64), rem = it - i * ((G + 1) * 64);
    const int hsel = rem >> 6, d = rem & 63;
    const int p = pos + i;
    const float c = bf2f(a.cos[(int64_t)p * 64 + d]), sn = bf2f(a.sin[(int64_t)p * 64 + d]);
    const bf16_t* row = qkv + (int64_t)i * a.qkv_ld;
    const bf16_t* src = hsel < G ? row + (kh * G + hsel) * 128 : row + (a.Hq + kh) * 128;
    float o1, o2;
    rope_pair(bf2f(src[d]), bf2f(src[d + 64]), c, sn, o1, o2);
    if (hsel < G) { qb[i * G + hsel][d] = f2bf(o1); qb[i * G + hsel][d + 64] = f2bf(o2); }
    else { kn[i][d] = f2bf(o1); kn[i][d + 64] = f2bf(o2); }
  }
  for (int it = tid; it < Tl * 128; it += 256) vn[it >> 7][it & 127] = qkv[(int64_t)(it >> 7) * a.qkv_ld + (a.Hq + a.Hkv + kh) * 128 + (it & 127)];
  for (int it = tid; it < (M - Tl * G) * 128; it += 256) qb[Tl * G + (it >> 7)][it & 127] = 0;
  __syncthreads();
  if (sp == 0) {   // designated writer of the new cache rows (positions pos .. last < ctx_max)
    bf16_t* kc = (bf16_t*)a.kcache + ((int64_t)kh * a.ctx_max + pos) * 128;
    bf16_t* vc = (bf16_t*)a.vcache + ((int64_t)kh * a.ctx_max + pos) * 128;
    for (int it = tid; it < Tl * 64; it += 256) {
      ((unsigned*)kc)[it] = ((const unsigned*)&kn[0][0])[it];
      ((unsigned*)vc)[it] = ((const unsigned*)&vn[0][0])[it];
    }
  }
  // ---- scores
  {
    bf16x8 qf[MB][4];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int s = 0; s < 4; ++s) qf[mb][s] = __builtin_bit_cast(bf16x8, *(const u32x4*)&qb[mb * 16 + lr][32 * s + 8 * lc]);
    for (int tb = tb0; tb < kend; tb += AV_KT) {
      const int key = tb + 16 * wave + lr;
      const bool own = key >= pos && key <= last;
      const bf16_t* kp = Kc + (int64_t)min(key, a.ctx_max - 1) * 128 + 8 * lc;     // (in bounds whatever the key; unused when masked)
      const bf16_t* op = &kn[own ? key - pos : 0][8 * lc];
      f32x4 acc[MB];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
      u32x4 kg[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) kg[s] = *(const u32x4*)(kp + 32 * s);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const u32x4 ko = *(const u32x4*)(op + 32 * s);
        u32x4 kv = own ? ko : kg[s];
        if (key > last) kv = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[mb][s], __builtin_bit_cast(bf16x8, kv), acc[mb], 0, 0, 0);
      }
      const int kk = tb - kbeg + 16 * wave + lr;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[mb * 16 + 4 * lc + r][kk] = acc[mb][r] * a.scale;
    }
  }
  __syncthreads();
  // ---- softmax: a wave per row, lanes over the split's keys in index order; P as bf16 (0 for a key the row does not see)
  const int kk0 = tb0 - kbeg;
  const int kkp = min(a.C, (kend - kbeg + AV_KT - 1) & ~(AV_KT - 1));      // whole tiles
  for (int r = wave; r < M; r += 4) {
    const bool live = r < Tl * G;
    const int i = r / G, p = pos + i;
    const int lo = av_lo(p, a.window);
    float m = -1e30f;
    for (int kk = kk0 + lane; kk < kkp; kk += 64) {
      const int key = kbeg + kk;
      if (live && key >= lo && key <= p) m = fmaxf(m, sc[r][kk]);
    }
    m = wave_max(m);
    float l = 0.f;
    for (int kk = kk0 + lane; kk < kkp; kk += 64) {
      const int key = kbeg + kk;
      float pe = 0.f;
      if (live && key >= lo && key <= p) pe = __expf(sc[r][kk] - m);
      l += pe;
      pb[r][kk] = f2bf(pe);
    }
    l = wave_sum(l);
    if (live && lane == 0) {
      const int64_t o = ((int64_t)i * a.Hq + kh * G + (r - i * G)) * NSP + sp;
      a.pm[o] = m;
      a.pl[o] = l;
    }
  }
  __syncthreads();
  // ---- PV: the V tile through LDS (own rows from vn, keys past `last` zero), a wave per 32 d, tiles in ascending order
  {
    f32x4 acc[MB][2];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto ldv = [&](int tb, u32x4 (&v)[4]) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = tid + 256 * u, row = q >> 4, c = q & 15;
        const int key = tb + row;
        const bool own = key >= pos && key <= last;
        const u32x4 g = *(const u32x4*)(Vc + (int64_t)min(key, a.ctx_max - 1) * 128 + c * 8);
        const u32x4 o = *(const u32x4*)&vn[own ? key - pos : 0][c * 8];
        v[u] = own ? o : g;
        if (key > last) v[u] = u32x4{0u, 0u, 0u, 0u};
      }
    };
    u32x4 cur[4], nxt[4];
    if (tb0 < kend) ldv(tb0, cur);
    for (int tb = tb0; tb < kend; tb += AV_KT) {
      const bool more = tb + AV_KT < kend;
      if (more) ldv(tb + AV_KT, nxt);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = tid + 256 * u;
        *(u32x4*)&vs[q >> 4][(q & 15) * 8] = cur[u];
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 pf[MB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) pf[mb] = __builtin_bit_cast(bf16x8, *(const u32x4*)&pb[mb * 16 + lr][tb - kbeg + 32 * ks + 8 * lc]);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          const int d = (2 * wave + nb) * 16 + lr;
          u32x4 vv;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            vv[e] = (unsigned)vs[32 * ks + 8 * lc + 2 * e][d] | ((unsigned)vs[32 * ks + 8 * lc + 2 * e + 1][d] << 16);
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[mb], __builtin_bit_cast(bf16x8, vv), acc[mb][nb], 0, 0, 0);
        }
      }
      __syncthreads();
      if (more) {
#pragma unroll
        for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
      }
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mb * 16 + 4 * lc + r;
        if (row >= Tl * G) continue;
        const int i = row / G;
        float* po = a.po + (((int64_t)i * a.Hq + kh * G + (row - i * G)) * NSP + sp) * 128;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) po[(2 * wave + nb) * 16 + lr] = acc[mb][nb][r];
      }
  }
