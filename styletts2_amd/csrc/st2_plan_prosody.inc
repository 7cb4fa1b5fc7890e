// Launch plan: alignment expansion + ProsodyPredictor.F0Ntrain.  Textually included by st2_engine.hip INSIDE its anonymous namespace (one translation unit:
// the plans share the packed-weight structs, the workspace arena and conv() defined there); split out per plan in round 6.

// ------------------------------------------------------------------------------------------------------------------
// prosody plan == the notebooks' alignment expansion + ProsodyPredictor.F0Ntrain (styletts2_amd/text.py, pipeline.py)
// ------------------------------------------------------------------------------------------------------------------
PLstm pack_lstm(Packer& pk, const std::string& prefix) {
  PLstm l;
  const HostTensor* wf = pk.get(prefix + ".weight_ih_l0");
  const HostTensor* wr = pk.get(prefix + ".weight_ih_l0_reverse");
  const HostTensor* hf = pk.get(prefix + ".weight_hh_l0");
  const HostTensor* hr = pk.get(prefix + ".weight_hh_l0_reverse");
  const HostTensor* bif = pk.get(prefix + ".bias_ih_l0");
  const HostTensor* bhf = pk.get(prefix + ".bias_hh_l0");
  const HostTensor* bir = pk.get(prefix + ".bias_ih_l0_reverse");
  const HostTensor* bhr = pk.get(prefix + ".bias_hh_l0_reverse");
  if (!wf || !wr || !hf || !hr || !bif || !bhf || !bir || !bhr) return l;
  if (wf->shape.size() != 2 || wf->shape[0] % 4 != 0) { pk.fail(prefix + ".weight_ih_l0 must be [4H, I]"); return l; }
  const int G4 = (int)wf->shape[0], I = (int)wf->shape[1], H = G4 / 4;
  for (const HostTensor* t : {wr})
    if (t->shape != wf->shape) { pk.fail(prefix + ": the two directions' input weights differ in shape"); return l; }
  for (const HostTensor* t : {hf, hr})
    if (t->shape.size() != 2 || t->shape[0] != G4 || t->shape[1] != H) { pk.fail(prefix + ".weight_hh_l0* must be [4H, H]"); return l; }
  for (const HostTensor* t : {bif, bhf, bir, bhr})
    if (t->numel() != G4) { pk.fail(prefix + ".bias_* must have 4H elements"); return l; }
  l.H = H;
  std::vector<float> w((size_t)2 * G4 * I);  // cat([W_ih, W_ih_reverse]) as a k = 1 conv weight [8H][I][1]
  std::copy(wf->data.begin(), wf->data.end(), w.begin());
  std::copy(wr->data.begin(), wr->data.end(), w.begin() + (size_t)G4 * I);
  l.w_ih = pack_split(pk.blob, prefix + ".weight_ih_l0", w.data(), 2 * G4, I, 1);
  std::vector<float> b((size_t)2 * G4);
  for (int i = 0; i < G4; ++i) {
    b[(size_t)i] = bif->data[(size_t)i] + bhf->data[(size_t)i];
    b[(size_t)G4 + i] = bir->data[(size_t)i] + bhr->data[(size_t)i];
  }
  l.bias = pk.blob.add_f32(b);
  std::vector<float> t((size_t)2 * H * G4);  // stack([W_hh.t(), W_hh_reverse.t()]): [2][H][4H]
  for (int dir = 0; dir < 2; ++dir) {
    const HostTensor* h = dir ? hr : hf;
    for (int r = 0; r < G4; ++r)
      for (int k = 0; k < H; ++k) t[((size_t)dir * H + k) * G4 + r] = h->data[(size_t)r * H + k];
  }
  l.whh_t = pk.blob.add_f32(t);
  return l;
}

int pack_predictor(st2_engine& e, Blob& blob, std::string* err) {
  const st2_model_config& cfg = e.cfg;
  Packer pk{e, blob};
  PPredictor p;
  Bank bank;
  const std::string P = "predictor.";
  const int dh = cfg.pred_hidden;
  if (dh <= 0) { *err = "st2_model_config.pred_hidden is not set"; return 1; }
  p.shared = pack_lstm(pk, P + "shared");
  // registration order of text.ProsodyPredictor._prepare: F0[0..2] then N[0..2], norm1 then norm2 each
  const int din[3] = {dh, dh, dh / 2}, dout[3] = {dh, dh / 2, dh / 2};
  for (int path = 0; path < 2; ++path) {
    for (int i = 0; i < 3; ++i) {
      const std::string pre = P + (path ? "N." : "F0.") + std::to_string(i);
      PAdainResBlk& r = path ? p.n[i] : p.f0[i];
      r = pack_adain_resblk(pk, pre, din[i], dout[i], i == 1);
      r.n1 = bank.add(pk, pre + ".norm1", din[i]);
      r.n2 = bank.add(pk, pre + ".norm2", dout[i]);
    }
  }
  p.f0p_w = pk.vec(P + "F0_proj.weight", dh / 2); p.f0p_b = pk.vec(P + "F0_proj.bias", 1);  // Conv1d(d_hid / 2, 1, 1)
  p.np_w = pk.vec(P + "N_proj.weight", dh / 2);   p.np_b = pk.vec(P + "N_proj.bias", 1);
  if (pk.ok && p.shared.H * 2 != dh) pk.fail(P + "shared: hidden size does not match st2_model_config.pred_hidden");
  if (!pk.ok) { *err = "predictor parameter missing or malformed: " + pk.missing; return 1; }
  p.J = bank.J;
  bank.pack(pk, cfg.style_dim, &p.bank_wt, &p.bank_b);
  p.ready = true;
  e.pred = p;
  return 0;
}

// asr[B][dim_in][T] = expand(t_en), (F0, N)[B][2T] = F0Ntrain(expand(d), s); d_cm [B][pred_hidden + style_dim][N] is the
// duration encoder's output channel-major, dur int64 [B][N] with rows summing to T
int prosody_plan(Ctx& c, const st2_engine& e, const float* d_cm, const float* t_en, const int64_t* dur, const float* s_p,
                 int B, int N, int T, int shift, float* asr, float* f0, float* nn, const int32_t* frames = nullptr) {
  const st2_model_config& cfg = e.cfg;
  const PPredictor& p = e.pred;
  const int dh = cfg.pred_hidden, Cd = dh + cfg.style_dim, Ct = cfg.dim_in;
  // ragged rows: T_b = frames[b] and 2 T_b (after the up-sampling block) per row
  const int32_t* lenT = nullptr;
  const int32_t* len2T = nullptr;
  if (frames) {
    const int32_t coef[6] = {1, 0, 1, 2, 0, 1};
    int32_t* tab = static_cast<int32_t*>(c.a.alloc((int64_t)2 * B * 4));
    RUN(c, g_be.ragged_lengths(frames, B, T, 2, coef, tab, c.stream));
    lenT = tab;
    len2T = tab + B;
  }
  View en = new_ncl(c, B, Cd, T, false).with_len(lenT);
  expand_by_durations(c, d_cm, N, dur, shift, en);  // ragged: exact zeros past T_b
  expand_by_durations(c, t_en, N, dur, shift, wrap(asr, B, Ct, T).with_len(lenT));
  // shared BiLSTM: input projection of every frame as one k = 1 conv, then the recurrence
  const int H = p.shared.H;
  View G = new_ncl(c, B, 8 * H, T, false).with_len(lenT);
  {
    ConvOpt o;
    o.bias = e.F(p.shared.bias);
    conv(c, e, en, p.shared.w_ih, G, o);
  }
  View y = new_ncl(c, B, 2 * H, T, false).with_len(lenT);
  const int64_t sb = st2_lstm_coop_scratch_bytes(B);
  void* scratch = sb > 0 ? c.a.alloc(sb) : nullptr;
  // packed-sequence semantics: row b's recurrence runs over its own T_b frames (frames = the lengths; NULL = T)
  RUN(c, g_be.lstm_bidir(G.p, G.bs, G.cs, e.F(p.shared.whh_t), lenT, B, H, T, y.p, y.bs, y.cs, scratch, sb, c.stream));
  float* h = c.a.f32((int64_t)B * p.J);
  RUN(c, g_be.style_fc(s_p, B, cfg.style_dim, e.F(p.bank_wt), e.F(p.bank_b), p.J, ST2_ACT_NONE, h, c.stream));
  DecRun r{c, e, h, p.J};
  r.lenT = lenT;
  r.len2T = len2T;
  for (int path = 0; path < 2; ++path) {
    const PAdainResBlk* blks = path ? p.n : p.f0;
    View t = y;
    for (int i = 0; i < 3; ++i) {
      View out = new_ncl(c, B, blks[i].dim_out, blks[i].upsample ? 2 * t.L : t.L, false);
      run_adain_resblk(r, blks[i], t, out);
      t = out.with_len(t.len && blks[i].upsample ? len2T : t.len);
    }
    float* dst = path ? nn : f0;
    // F0 / N; ragged: exact zeros past 2 T_b
    conv1d_direct(c, t, e.F(path ? p.np_w : p.f0p_w), e.F(path ? p.np_b : p.f0p_b), wrap(dst, B, 1, t.L).with_len(t.len), 1, 1, 0);
  }
  return c.rc;
}
