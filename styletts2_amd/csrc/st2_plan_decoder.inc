// Launch plan: Decoder.forward + Generator (iSTFTNet / HiFi-GAN).  Textually included by st2_engine.hip INSIDE its anonymous namespace (one translation unit:
// the plans share the packed-weight structs, the workspace arena and conv() defined there); split out per plan in round 6.

// ------------------------------------------------------------------------------------------------------------------
// decoder plan == styletts2_amd/decoder.py
// ------------------------------------------------------------------------------------------------------------------
struct DecRun {
  Ctx& c;
  const st2_engine& e;
  const float* h;  // style bank output [B][J]
  int J;
  const int32_t* lenT = nullptr;   // ragged plans: per-row frame counts T_b ...
  const int32_t* len2T = nullptr;  // ... and 2 T_b (the up-sampling AdainResBlk1d maps one to the other)
  const float* gamma(int off) const { return h + off; }
  const float* beta(int off, int channels) const { return h + off + channels; }
};

// AdaINResBlock1.forward (Modules/istftnet.py:66-75); the MRF sum / division ride in the last conv's epilogue
View run_resblock1(DecRun& r, const PResBlock1& p, View x, const float* x_stats, View mrf_acc, bool mrf_last, int n_mrf,
                   View out) {
  Ctx& c = r.c;
  const int C = p.channels, ks = p.ks, B = x.B, L = x.L;
  const float* st = x_stats;
  if (!st) {
    float* s0 = new_stats(c, B, C);
    instnorm_stats(c, x, s0);
    st = s0;
  }
  // ragged rows: every intermediate ends where the block's input does
  View xt = new_ncl(c, B, C, L).with_len(x.len);
  View ping[2] = {new_ncl(c, B, C, L).with_len(x.len), new_ncl(c, B, C, L).with_len(x.len)};
  float* st2 = new_stats(c, B, C);
  float* stn[2] = {new_stats(c, B, C), new_stats(c, B, C)};
  for (int i = 0; i < 3; ++i) {
    const int d = p.dil[i];
    ConvOpt o1;
    o1.dil = d; o1.pad_left = (ks * d - d) / 2; o1.bias = r.e.F(p.c1[i].bias); o1.pro = ST2_PRO_ADAIN_SNAKE;
    o1.stats = st; o1.gamma = r.gamma(p.ad1[i]); o1.beta = r.beta(p.ad1[i], C); o1.gb_bs = r.J;
    o1.alpha = r.e.F(p.a1[i]); o1.stats_out = st2;
    conv(c, r.e, x, p.c1[i].w, xt, o1);
    const bool last = i == 2;
    ConvOpt o2;
    o2.dil = 1; o2.pad_left = (ks - 1) / 2; o2.bias = r.e.F(p.c2[i].bias); o2.pro = ST2_PRO_ADAIN_SNAKE;
    o2.stats = st2; o2.gamma = r.gamma(p.ad2[i]); o2.beta = r.beta(p.ad2[i], C); o2.gb_bs = r.J;
    o2.alpha = r.e.F(p.a2[i]); o2.res = x;
    if (last) {
      o2.res2 = mrf_acc;
      o2.div = mrf_last ? (float)n_mrf : 1.0f;
      conv(c, r.e, xt, p.c2[i].w, out, o2);
      x = out;
    } else {
      o2.stats_out = stn[i & 1];
      conv(c, r.e, xt, p.c2[i].w, ping[i & 1], o2);
      x = ping[i & 1];
      st = stn[i & 1];
    }
  }
  return x;
}

// AdainResBlk1d.forward (Modules/istftnet.py:435-454): (residual(x, s) + shortcut(x)) / sqrt(2)
void run_adain_resblk(DecRun& r, const PAdainResBlk& p, const View& x, const View& out_in) {
  Ctx& c = r.c;
  const int B = x.B, L = x.L;
  const int64_t mark = c.a.off;
  // ragged rows: x ends at T_b (or 2 T_b), the output at the same or -- up-sampling -- twice that
  const int32_t* len_o = x.len;
  if (x.len && p.upsample) {
    if (x.len != r.lenT && c.rc == 0) { st2_set_error("engine: ragged up-sampling block on rows of unknown length"); c.rc = 1; }
    len_o = r.len2T;
  }
  const View out = out_in.with_len(len_o);
  float* st1 = new_stats(c, B, p.dim_in);
  instnorm_stats(c, x.rows(0, p.dim_in), st1);
  float* st2 = new_stats(c, B, p.dim_out);
  const int Lo = p.upsample ? 2 * L : L;
  View t1 = new_ncl(c, B, p.dim_out, Lo).with_len(len_o);
  if (p.upsample) {
    View u = new_ncl(c, B, p.dim_in, 2 * L).with_len(len_o);
    adain_leaky_pool(c, x.rows(0, p.dim_in), st1, r.gamma(p.n1), r.beta(p.n1, p.dim_in), r.J, 0.2f, r.e.F(p.pool_w),
                     r.e.F(p.pool_b), u);
    ConvOpt o;
    o.pad_left = 1; o.bias = r.e.F(p.conv1.bias); o.stats_out = st2;
    conv(c, r.e, u, p.conv1.w, t1, o);
  } else {
    ConvOpt o;
    o.pad_left = 1; o.bias = r.e.F(p.conv1.bias); o.pro = ST2_PRO_ADAIN_LEAKY; o.slope = 0.2f; o.stats = st1;
    o.gamma = r.gamma(p.n1); o.beta = r.beta(p.n1, p.dim_in); o.gb_bs = r.J; o.stats_out = st2;
    conv(c, r.e, x, p.conv1.w, t1, o);
  }
  View sc = x;
  if (p.learned_sc) {  // the 1x1 shortcut commutes with nearest x2 up-sampling: it runs at the low rate
    sc = new_ncl(c, B, p.dim_out, L).with_len(x.len);
    ConvOpt o;
    conv(c, r.e, x, p.sc.w, sc, o);
  }
  ConvOpt o;
  o.pad_left = 1; o.bias = r.e.F(p.conv2.bias); o.pro = ST2_PRO_ADAIN_LEAKY; o.slope = 0.2f; o.stats = st2;
  o.gamma = r.gamma(p.n2); o.beta = r.beta(p.n2, p.dim_out); o.gb_bs = r.J; o.res = sc;
  o.res_shift = p.upsample ? 1 : 0;
  o.div = (float)sqrt(2.0);  // python passes math.sqrt(2) through a c_float: the same fp32 value
  conv(c, r.e, t1, p.conv2.w, out, o);
  c.a.off = mark;
}

void tap(Ctx& c, const View& v, float* dst) {
  if (!dst) return;
  RUN(c, g_be.copy_ncl(v.p, v.bs, v.cs, dst, (int64_t)v.C * v.L, v.L, v.B, v.C, v.L, c.stream));
}

// Per-row lengths of the ragged decoder plan, all affine in the row's frame count: (mul * T_b + add) / div
struct DecLens {
  enum { T1 = 0, T2, SAMPLES, HAR, STAGE0 };  // stage i: STAGE0 + 3 i = output, + 1 = ConvTranspose phase columns, + 2 = noise-conv input
  std::vector<int32_t> coef;
  int add(long long mul, long long a, long long div = 1) {
    coef.push_back((int32_t)mul); coef.push_back((int32_t)a); coef.push_back((int32_t)div);
    return (int)coef.size() / 3 - 1;
  }
};

int decoder_plan(Ctx& c, const st2_engine& e, const float* asr_p, const float* f0_p, const float* n_p, const float* s_p,
                 const float* sine_noise, const float* har_inject, int B, int T, float* wave,
                 const st2_decoder_taps* taps, const int32_t* frames = nullptr) {
  const st2_model_config& cfg = e.cfg;
  const PDecoder& d = e.dec;
  const PGenerator& g = d.gen;
  const bool ist = cfg.decoder_kind == 0;
  const int Cin = cfg.dim_in, nu = cfg.n_upsamples, nk = cfg.n_resblock_kernels;
  const int T2 = 2 * T;
  st2_decoder_taps notaps;
  memset(&notaps, 0, sizeof(notaps));
  if (!taps) taps = &notaps;

  // ragged rows: every per-row length of the plan from `frames` in one launch (the solo formulas, row by row)
  const int hop_ = cfg.gen_istft_hop;
  const int up_ = prod_from(cfg.upsample_rates, 0, nu) * (ist ? hop_ : 1);
  const int32_t* lens = nullptr;
  auto len_of = [&](int i) -> const int32_t* { return lens ? lens + (int64_t)i * B : nullptr; };
  if (frames) {
    if (nu > 4) { st2_set_error("engine: ragged decoder supports up to 4 up-sampling stages"); return 1; }
    static_assert(DecLens::STAGE0 + 3 * 4 <= 16, "st2_decoder_workspace_bytes sizes a table of 16 lengths");
    DecLens dl;
    dl.add(1, 0); dl.add(2, 0); dl.add(2LL * up_, 0);
    if (ist) dl.add(2LL * up_, hop_, hop_);  // istftnet: 120 T_b + 1 STFT frames
    else dl.add(2LL * up_, 0);               // hifigan: the samples themselves
    long long m = 2, a = 0;  // stage input 2 T_b
    long long hm = 2LL * up_ / (ist ? hop_ : 1), ha = ist ? 1 : 0;  // harmonic features
    for (int i = 0; i < nu; ++i) {
      const int u = cfg.upsample_rates[i], k = cfg.upsample_kernel_sizes[i];
      const int pad = ist ? (k - u) / 2 : u / 2 + u % 2;
      const int extra = ist ? 0 : u % 2;
      const int refl = (ist && i + 1 == nu) ? 1 : 0;
      const long long m_o = m * u, a_o = (a - 1) * u - 2 * pad + k + extra + refl;
      dl.add(m_o, a_o);
      dl.add(m, a + 1);  // the ConvTranspose GEMM's L_in + 1 columns
      const int sf = g.noise_stride[i];
      if (sf > 1) {
        const int pf = (sf + 1) / 2;
        dl.add(hm, ha + 2 * pf - 2 * sf + sf + sf, sf);  // L_ns + 1 = (L_har + 2 pf - 2 sf) / sf + 2
      } else {
        dl.add(hm, ha);
      }
      m = m_o; a = a_o;
    }
    int32_t* tab = static_cast<int32_t*>(c.a.alloc((int64_t)dl.coef.size() / 3 * B * 4));
    RUN(c, g_be.ragged_lengths(frames, B, T, (int)dl.coef.size() / 3, dl.coef.data(), tab, c.stream));
    lens = tab;
  }

  float* h = c.a.f32((int64_t)B * d.J);
  RUN(c, g_be.style_fc(s_p, B, cfg.style_dim, e.F(d.bank_wt), e.F(d.bank_b), d.J, ST2_ACT_NONE, h, c.stream));
  DecRun r{c, e, h, d.J};
  r.lenT = len_of(DecLens::T1);
  r.len2T = len_of(DecLens::T2);

  View asr = wrap(asr_p, B, Cin, T).with_len(r.lenT);
  View f0 = wrap(f0_p, B, 1, T2).with_len(r.len2T), nn = wrap(n_p, B, 1, T2).with_len(r.len2T);
  // [x(1024) | asr_res(64) | F0 | N] lives in one buffer; producers write their channel slices in place
  View cat = new_ncl(c, B, 1024 + 64 + 2, T, false).with_len(r.lenT);
  View cat0 = new_ncl(c, B, Cin + 2, T, false).with_len(r.lenT);
  RUN(c, g_be.copy_ncl(asr.p, asr.bs, asr.cs, cat0.p, cat0.bs, cat0.cs, B, Cin, T, c.stream));
  {
    // ragged rows: F0 / N end at 2 T_b, the stride-2 convs see their zero padding there; their outputs are not cut
    View a = cat0.rows(Cin, Cin + 1).with_len(nullptr), b = cat0.rows(Cin + 1, Cin + 2).with_len(nullptr);
    conv1d_direct(c, f0, e.F(d.f0_w), e.F(d.f0_b), a, 3, 2, 1);
    conv1d_direct(c, nn, e.F(d.n_w), e.F(d.n_b), b, 3, 2, 1);
    View src = cat0.rows(Cin, Cin + 2), dst = cat.rows(1088, 1090);
    RUN(c, g_be.copy_ncl(src.p, src.bs, src.cs, dst.p, dst.bs, dst.cs, B, 2, T, c.stream));
  }
  {
    ConvOpt o;
    o.bias = e.F(d.asr_res.bias);
    conv(c, e, asr, d.asr_res.w, cat.rows(1024, 1088), o);
  }
  run_adain_resblk(r, d.encode, cat0, cat.rows(0, 1024));
  tap(c, cat.rows(0, 1024), taps->encode);
  View x = new_ncl(c, B, 512, T2).with_len(r.len2T);
  for (int i = 0; i < 4; ++i) {
    if (d.decode[i].upsample)
      run_adain_resblk(r, d.decode[i], cat, x);
    else
      run_adain_resblk(r, d.decode[i], cat, cat.rows(0, 1024));
  }
  tap(c, x, taps->front);

  // ---- generator (istftnet.py:350-380 / hifigan.py:321-347) ---------------------------------------------------------
  int up_scale = prod_from(cfg.upsample_rates, 0, nu) * (ist ? cfg.gen_istft_hop : 1);
  const int L = T2 * up_scale;  // samples
  const int n_fft = cfg.gen_istft_n_fft, hop = cfg.gen_istft_hop;
  View har;
  if (har_inject) {
    har = ist ? wrap(har_inject, B, n_fft + 2, L / hop + 1) : wrap(har_inject, B, 1, L);
  } else {
    float* scratch = c.a.f32((int64_t)B * 9 * T2);
    float* hs = c.a.f32((int64_t)B * L);
    har_source(c, f0_p, B, T2, up_scale, sine_noise, e.F(g.lin_w), e.F(g.lin_b), scratch, hs, r.len2T);  // ragged: 600 T_b samples
    if (taps->har_source) RUN(c, g_be.copy_ncl(hs, L, L, taps->har_source, L, L, B, 1, L, c.stream));
    if (ist) {
      har = new_ncl(c, B, n_fft + 2, L / hop + 1, false);
      stft_mag_phase(c, hs, L, n_fft, hop, har, len_of(DecLens::SAMPLES));  // ragged: phase_split then needs no lengths
    } else {
      har = wrap(hs, B, 1, L);
    }
  }
  har = har.with_len(len_of(DecLens::HAR));
  if (ist) tap(c, har, taps->har);

  for (int i = 0; i < nu; ++i) {
    const int u = cfg.upsample_rates[i], k = cfg.upsample_kernel_sizes[i], C = g.channels[i];
    const bool last = i + 1 == nu;
    const int L_in = x.L;
    int pad, L_raw;
    if (ist) {
      pad = (k - u) / 2;
      L_raw = (L_in - 1) * u - 2 * ((k - u) / 2) + k;
    } else {
      pad = u / 2 + u % 2;
      L_raw = (L_in - 1) * u - 2 * (u / 2 + u % 2) + k + u % 2;
    }
    const bool reflect = ist && last;
    const int L_out = L_raw + (reflect ? 1 : 0);
    const int32_t* len_o = len_of(DecLens::STAGE0 + 3 * i);  // ragged rows: this stage's per-row output length
    // persistent across the stage: the stage output and the MRF accumulators
    View x_next = new_ncl(c, B, C, L_out).with_len(len_o);
    const int64_t stage_mark = c.a.off;
    // harmonic-source branch (istftnet.py:361-362 / hifigan.py:330-331)
    View xs_src = new_ncl(c, B, C, L_out).with_len(len_o);
    {
      const int64_t m = c.a.off;
      View xs0 = new_ncl(c, B, C, L_out).with_len(len_o);
      const int stride_f0 = g.noise_stride[i];
      ConvOpt o;
      o.bias = e.F(g.noise_b[i]);
      if (stride_f0 > 1) {
        const int pad_f0 = (stride_f0 + 1) / 2;
        const int L_ns = (har.L + 2 * pad_f0 - 2 * stride_f0) / stride_f0 + 1;
        View harp = new_ncl(c, B, har.C * stride_f0, L_ns + 1, false).with_len(len_of(DecLens::STAGE0 + 3 * i + 2));
        RUN(c, g_be.phase_split(har.p, har.bs, har.cs, B, har.C, har.L, stride_f0, pad_f0, harp.p, harp.bs, harp.cs,
                                L_ns + 1, c.stream));
        if (L_ns != L_out && c.rc == 0) { st2_set_error("engine: noise conv length %d != stage length %d", L_ns, L_out); c.rc = 1; }
        conv(c, e, harp, g.noise_wt[i], xs0, o);
      } else {
        conv(c, e, har, g.noise_wt[i], xs0, o);
      }
      View nul;
      run_resblock1(r, g.noise_res[i], xs0, nullptr, nul, false, nk, xs_src);
      // xs_src was allocated before m: keep it, drop the branch temporaries
      c.a.off = m;
    }
    // up-sampling ConvTranspose1d as polyphase GEMM + interleave (istftnet.py:360,364-368)
    View xu = new_ncl(c, B, C, L_out).with_len(len_o);
    float* st = new_stats(c, B, C);
    {
      const int64_t m = c.a.off;
      View Y = new_ncl(c, B, u * C, L_in + 1).with_len(len_of(DecLens::STAGE0 + 3 * i + 1));
      ConvOpt o;
      o.pad_left = 1;
      if (ist) { o.pro = ST2_PRO_LEAKY; o.slope = 0.1f; } else { o.pro = ST2_PRO_SNAKE; o.alpha = e.F(g.alphas[i]); }
      conv(c, e, x, g.ups_wt[i], Y, o);
      const int tile = st2_convt_interleave_part_cols(), nt = (L_out + tile - 1) / tile;
      float* part = c.a.f32((int64_t)B * C * nt * 3);
      convt_interleave_stats(c, Y, e.F(g.ups_b[i]), xs_src, xu, u, pad, L_raw, reflect ? 1 : 0, part, nt);
      finalize_stats(c, part, xu, nt, st, tile);
      c.a.off = m;
    }
    // multi-receptive-field fusion (istftnet.py:369-375): ((r0 + r1) + r2) / n in the last convs' epilogues
    View acc[2] = {new_ncl(c, B, C, L_out).with_len(len_o), new_ncl(c, B, C, L_out).with_len(len_o)};
    View prev;
    for (int j = 0; j < nk; ++j) {
      const int64_t m = c.a.off;
      const bool lastk = j + 1 == nk;
      View out = lastk ? x_next : acc[j & 1];
      run_resblock1(r, g.resblocks[(size_t)i * nk + j], xu, st, prev, lastk, nk, out);
      prev = out;
      c.a.off = m;
    }
    x = x_next;
    c.a.off = stage_mark;
    if (i < 4) tap(c, x, taps->stage[i]);
  }
  if (ist) {
    const int nb = n_fft / 2 + 1;
    View sp = new_ncl(c, B, n_fft + 2, x.L, false).with_len(x.len);
    ConvOpt o;
    o.pad_left = 3; o.bias = e.F(g.post.bias); o.pro = ST2_PRO_LEAKY; o.slope = 0.01f; o.act = ST2_ACT_EXP_SIN;
    o.act_split = nb;
    conv(c, e, x, g.post.w, sp, o);
    tap(c, sp, taps->spec_phase);
    istft(c, sp, n_fft, hop, wave, (int64_t)hop * (x.L - 1));  // ragged: 600 T_b samples per row
  } else {
    View w = wrap(wave, B, 1, x.L).with_len(x.len);
    ConvOpt o;
    o.pad_left = 3; o.bias = e.F(g.post.bias); o.pro = ST2_PRO_SNAKE; o.alpha = e.F(g.alphas[(size_t)nu]);
    o.act = ST2_ACT_TANH;
    conv(c, e, x, g.post.w, w, o);
    if (frames) RUN(c, g_be.mask_tail(w.p, w.bs, w.cs, B, 1, w.L, w.len, c.stream));  // exact zeros past 600 T_b
  }
  return c.rc;
}
