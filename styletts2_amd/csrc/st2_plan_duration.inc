// Launch plan: DurationEncoder + duration head.  Textually included by st2_engine.hip INSIDE its anonymous namespace (one translation unit:
// the plans share the packed-weight structs, the workspace arena and conv() defined there); split out per plan in round 6.

// ------------------------------------------------------------------------------------------------------------------
// duration plan == DurationEncoder.forward + pipeline.predict_durations (styletts2_amd/text.py, pipeline.py)
// ------------------------------------------------------------------------------------------------------------------
int pack_duration(st2_engine& e, Blob& blob, std::string* err) {
  Packer pk{e, blob};
  PDuration d;
  const std::string T = "predictor.text_encoder.lstms.";
  for (int i = 0; pk.has(T + std::to_string(2 * i) + ".weight_ih_l0"); ++i) {
    d.lstms.push_back(pack_lstm(pk, T + std::to_string(2 * i)));
    const int dm = 2 * d.lstms.back().H;  // AdaLayerNorm(style_dim, d_model): fc = Linear(style_dim, 2 * d_model)
    d.ada_wt.push_back(pk.lin_t(T + std::to_string(2 * i + 1) + ".fc.weight", 2 * dm, e.cfg.style_dim));
    d.ada_b.push_back(pk.vec(T + std::to_string(2 * i + 1) + ".fc.bias", 2 * dm));
  }
  if (d.lstms.empty()) { *err = "missing predictor parameter predictor.text_encoder.lstms.0.weight_ih_l0"; return 1; }
  d.dur_lstm = pack_lstm(pk, "predictor.lstm");
  const HostTensor* pw = pk.get("predictor.duration_proj.linear_layer.weight", {-1, 2 * d.dur_lstm.H});
  d.proj_w = pk.vec("predictor.duration_proj.linear_layer.weight");
  if (pw) d.proj_b = pk.vec("predictor.duration_proj.linear_layer.bias", pw->shape[0]);
  if (!pk.ok || !pw) { *err = "predictor parameter missing or malformed: " + pk.missing; return 1; }
  d.max_dur = (int)pw->shape[0];
  d.ready = true;
  e.dur = d;
  return 0;
}

View lstm_run(Ctx& c, const st2_engine& e, const PLstm& l, const View& x, const int32_t* lens) {
  View G = new_ncl(c, x.B, 8 * l.H, x.L, false);
  ConvOpt o;
  o.bias = e.F(l.bias);
  conv(c, e, x, l.w_ih, G, o);
  View y = new_ncl(c, x.B, 2 * l.H, x.L, false);
  const int64_t sb = st2_lstm_coop_scratch_bytes(x.B);
  void* scratch = sb > 0 ? c.a.alloc(sb) : nullptr;
  RUN(c, g_be.lstm_bidir(G.p, G.bs, G.cs, e.F(l.whh_t), lens, x.B, l.H, x.L, y.p, y.bs, y.cs, scratch, sb, c.stream));
  return y;
}

int duration_plan(Ctx& c, const st2_engine& e, const View& d_en, const float* s_p, const int32_t* lens, int B, int N,
                  int tail, float* d_cm, int64_t* durations, const float* speed = nullptr, const float* tok_speed = nullptr) {
  const st2_model_config& cfg = e.cfg;
  const PDuration& d = e.dur;
  const int dh = cfg.pred_hidden, sty = cfg.style_dim, Cd = dh + sty;
  const int nl = (int)d.lstms.size();
  View h = new_ncl(c, B, Cd, N, false);
  {  // [x | style broadcast over the tokens], pad positions zeroed
    View src = d_en, dst = h.rows(0, dh), st = h.rows(dh, Cd);
    RUN(c, g_be.copy_ncl(src.p, src.bs, src.cs, dst.p, dst.bs, dst.cs, B, dh, N, c.stream));
    RUN(c, g_be.broadcast_cols(s_p, sty, st.p, st.bs, st.cs, B, sty, N, c.stream));
    if (lens) RUN(c, g_be.mask_tail(h.p, h.bs, h.cs, B, Cd, N, lens, c.stream));
  }
  for (int i = 0; i < nl; ++i) {
    View y = lstm_run(c, e, d.lstms[(size_t)i], h, lens);  // [B][dh][N]
    // AdaLayerNorm (models.py:418-438): (1 + gamma) * LayerNorm_c(y) + beta, gamma | beta = fc(style)
    float* gb = c.a.f32((int64_t)B * 2 * dh);
    RUN(c, g_be.style_fc(s_p, B, sty, e.F(d.ada_wt[(size_t)i]), e.F(d.ada_b[(size_t)i]), 2 * dh, ST2_ACT_NONE, gb, c.stream));
    float* st = c.a.f32((int64_t)B * N * 2);
    RUN(c, g_be.colnorm_stats(y.p, y.bs, y.cs, B, dh, N, 1e-5f, st, c.stream));
    const bool last = i + 1 == nl;
    View nh = last ? wrap(d_cm, B, Cd, N) : new_ncl(c, B, Cd, N, false);
    View top = nh.rows(0, dh), bot = nh.rows(dh, Cd);
    RUN(c, g_be.colnorm_apply(y.p, y.bs, y.cs, st, gb, gb + dh, 2 * dh, 1, ST2_ACT_NONE, 0.f, lens, top.p, top.bs, top.cs, B,
                              dh, N, c.stream));
    RUN(c, g_be.broadcast_cols(s_p, sty, bot.p, bot.bs, bot.cs, B, sty, N, c.stream));
    if (lens) RUN(c, g_be.mask_tail(bot.p, bot.bs, bot.cs, B, sty, N, lens, c.stream));
    h = nh;
  }
  if (durations) {
    View x = lstm_run(c, e, d.dur_lstm, h, lens);
    if (tok_speed)  // per-token rate on top of the row's (st2_front_forward_tok): the third instantiation, no backend slot
      RUN(c, st2_duration_head_rate_tok(x.p, x.bs, x.cs, e.F(d.proj_w), e.F(d.proj_b), B, dh, d.max_dur, N, lens, tail, speed,
                                        tok_speed, durations, nullptr, c.stream));
    else if (speed)  // per-row speaking rate (st2_front_forward_ctl): the twin kernel, no backend slot
      RUN(c, st2_duration_head_rate(x.p, x.bs, x.cs, e.F(d.proj_w), e.F(d.proj_b), B, dh, d.max_dur, N, lens, tail, speed,
                                    durations, nullptr, c.stream));
    else
      RUN(c, g_be.duration_head(x.p, x.bs, x.cs, e.F(d.proj_w), e.F(d.proj_b), B, dh, d.max_dur, N, lens, tail, durations,
                                nullptr, c.stream));
  }
  return c.rc;
}
