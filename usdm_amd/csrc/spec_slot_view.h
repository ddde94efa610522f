// The head of the batched speculative commit kernels (spec_k.hip), included as text: from `ba` (usdm_spec_batch_args) and `bst` (the
// batched usdm_decode_state) to `a` and `st` of slot b = slot_lo + blockIdx.x alone - every array moved on by b slots - and that
// slot's h_out rows; r0 = the slot's first row.
  const int b = ba.slot_lo + blockIdx.x;
  usdm_spec_args a = ba.s;
  usdm_decode_state st = bst;
  const int64_t r0 = (int64_t)b * a.T;
  if (a.part_val) { a.part_val += r0 * a.nparts; a.part_idx += r0 * a.nparts; }
  a.drafts += b * SP_TMAX;
  a.limit += b;
  if (a.prompt) a.prompt += (int64_t)b * a.prompt_max;
  a.prompt_len += b;
  if (a.script) a.script += (int64_t)b * st.max_out;
  a.counters += b * 3;
  st.next_token += b;
  st.out_tokens += (int64_t)b * st.max_out;
  st.step += b;
  st.pos += b;
  st.done += b;
  if (st.eos) st.eos += b * 8;
  h_out += r0 * Hd;
