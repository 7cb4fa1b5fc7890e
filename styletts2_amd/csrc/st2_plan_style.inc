// Launch plan: StyleEncoder.forward (both encoders).  Textually included by st2_engine.hip INSIDE its anonymous namespace (one translation unit:
// the plans share the packed-weight structs, the workspace arena and conv() defined there); split out per plan in round 6.

// ------------------------------------------------------------------------------------------------------------------
// style-encoder plan == StyleEncoder.forward (styletts2_amd/style.py): feature maps stored (h, c, w) with one zero row
// above and below, every 3x3 Conv2d one split-f16 Conv1d over the width with 3 stacked rows as its input channels
// ------------------------------------------------------------------------------------------------------------------
constexpr int STYLE_ZEROS = 4096;

// Conv2d weight [Co][Ci][kh][kw] -> Conv1d weight [Co][kh*Ci][kw] on kh stacked image rows (channel index dh*Ci + ci)
std::vector<float> rows_as_channels(const HostTensor& t) {
  const int co = (int)t.shape[0], ci = (int)t.shape[1], kh = (int)t.shape[2], kw = (int)t.shape[3];
  std::vector<float> v((size_t)co * kh * ci * kw);
  for (int o = 0; o < co; ++o)
    for (int i = 0; i < ci; ++i)
      for (int dh = 0; dh < kh; ++dh)
        for (int x = 0; x < kw; ++x)
          v[(((size_t)o * kh + dh) * ci + i) * kw + x] = t.data[(((size_t)o * ci + i) * kh + dh) * kw + x];
  return v;
}

int pack_style(st2_engine& e, Blob& blob, int which, std::string* err) {
  Packer pk{e, blob};
  PStyleEnc s;
  const std::string R = which == 0 ? "style_encoder." : "predictor_encoder.";
  auto conv2d = [&](const std::string& name) -> SplitW {  // folded Conv2d -> packed Conv1d over stacked rows
    const HostTensor* t = pk.get(name);
    if (!t || t->shape.size() != 4) { pk.ok = false; if (pk.missing.empty()) pk.missing = name + " (4-D expected)"; return SplitW(); }
    const std::vector<float> v = rows_as_channels(*t);
    return pack_split(blob, name, v.data(), (int)t->shape[0], (int)(t->shape[1] * t->shape[2]), (int)t->shape[3]);
  };
  const HostTensor* first = pk.get(R + "shared.0.weight");
  if (!first || first->shape.size() != 4 || first->shape[1] != 1 || first->shape[2] != 3 || first->shape[3] != 3) {
    *err = "missing or malformed style-encoder parameter " + R + "shared.0.weight (spectral norm folded by the caller)";
    return 1;
  }
  s.c0 = (int)first->shape[0];
  s.w0 = blob.add_f32(rows_as_channels(*first));  // [C0][3][3]: plain OIK for st2_conv1d_direct
  s.b0 = pk.vec(R + "shared.0.bias");
  int i = 1;
  for (; pk.has(R + "shared." + std::to_string(i) + ".conv1.weight"); ++i) {
    const std::string Bn = R + "shared." + std::to_string(i);
    PStyleBlk b;
    const HostTensor* w1 = pk.get(Bn + ".conv1.weight");
    const HostTensor* w2 = pk.get(Bn + ".conv2.weight");
    const HostTensor* wd = pk.get(Bn + ".downsample_res.conv.weight");
    if (!w1 || !w2 || !wd) break;
    if (w1->shape.size() != 4 || w2->shape.size() != 4 || w1->shape[0] != w1->shape[1] || w2->shape[1] != w1->shape[0] ||
        wd->numel() != w1->shape[0] * 9) {
      *err = "malformed style-encoder block " + Bn + " (ResBlk: conv1 [C, C, 3, 3], conv2 [C', C, 3, 3], depthwise [C, 1, 3, 3])";
      return 1;
    }
    b.c_in = (int)w1->shape[1];
    b.c_out = (int)w2->shape[0];
    b.w1 = conv2d(Bn + ".conv1.weight");  b.b1 = pk.vec(Bn + ".conv1.bias");
    b.w2 = conv2d(Bn + ".conv2.weight");  b.b2 = pk.vec(Bn + ".conv2.bias");
    b.wd = blob.add_f32(wd->data);        b.bd = pk.vec(Bn + ".downsample_res.conv.bias");  // [C][1][3][3] == [C][3][3]
    if (pk.has(Bn + ".conv1x1.weight")) {
      b.wsc = conv2d(Bn + ".conv1x1.weight");
      b.has_sc = true;
    }
    s.blocks.push_back(b);
  }
  // shared.{i} = LeakyReLU, shared.{i+1} = the 5x5 valid conv (models.py:151-153)
  const std::string last = R + "shared." + std::to_string(i + 1);
  s.w5 = conv2d(last + ".weight");
  s.b5 = pk.vec(last + ".bias");
  s.c_last = s.w5.C_out;
  s.wl = pk.conv_w(R + "unshared.weight");
  s.bl = pk.vec(R + "unshared.bias");
  s.style_dim = s.wl.C_out;
  if (!pk.ok || s.c0 > STYLE_ZEROS || s.c_last > STYLE_ZEROS) {
    *err = "style-encoder parameter missing or malformed: " + pk.missing;
    return 1;
  }
  if (s.blocks.size() != 4 || s.w5.ks != 5 || s.w5.C_in != 5 * s.blocks.back().c_out) {  // 80 mel bins -> 5 rows -> 5x5 valid conv
    *err = "style encoder " + R + ": expected four down-sampling ResBlks and a 5x5 valid conv (models.py:139-164)";
    return 1;
  }
  s.ready = true;
  e.style[which] = s;
  return 0;
}

int style_plan(Ctx& c, const st2_engine& e, const PStyleEnc& s, const float* mel, int B, int H, int W, float* out) {
  // [B][h + 2][ch][w] map whose rows 0 and h + 1 are zero (the rows 1 .. h are written by the producing kernel)
  auto new_map = [&](int h, int ch, int w) -> float* {
    float* p = c.a.f32((int64_t)B * (h + 2) * ch * w);
    for (int r : {0, h + 1})
      RUN(c, g_be.broadcast_cols(e.F(e.zeros), 0, p + (int64_t)r * ch * w, (int64_t)(h + 2) * ch * w, w, B, ch, w, c.stream));
    return p;
  };
  // rows r0 .. r0 + k - 1 of utterance b's padded map stacked along the channels: [h][k * ch][w] (overlapping view)
  auto rows = [&](float* P, int b, int h, int ch, int w, int k, int r0) {
    View v;
    v.p = P + (int64_t)b * (h + 2) * ch * w + (int64_t)r0 * ch * w;
    v.B = h; v.C = k * ch; v.L = w; v.bs = (int64_t)ch * w; v.cs = w;  // k = 3 from row 0 / k = 1 from row 1: h image rows
    return v;
  };
  auto plain = [&](float* p, int b, int h, int ch, int w) {  // [h][ch][w] of utterance b in an unpadded [B][h][ch][w] buffer
    View v;
    v.p = p + (int64_t)b * h * ch * w;
    v.B = h; v.C = ch; v.L = w; v.bs = (int64_t)ch * w; v.cs = w;
    return v;
  };
  float* m0 = new_map(H, 1, W);
  RUN(c, g_be.copy_ncl(mel, (int64_t)H * W, W, m0 + W, (int64_t)(H + 2) * W, W, B, H, W, c.stream));
  int C = s.c0;
  float* P = new_map(H, C, W);
  for (int b = 0; b < B; ++b) {
    const View x = rows(m0, b, H, 1, W, 3, 0);
    RUN(c, g_be.conv1d_direct(x.p, x.bs, x.cs, e.F(s.w0), e.F(s.b0), P + (int64_t)b * (H + 2) * C * W + (int64_t)C * W,
                              (int64_t)C * W, W, H, 3, C, W, W, 3, 1, 1, c.stream));
  }
  for (const PStyleBlk& blk : s.blocks) {
    const int Co = blk.c_out, Ho = H / 2, Wo = (W + 1) / 2;
    // shortcut: 1x1 conv at full resolution, then the 2x2 average (models.py:118-123)
    float* SC = c.a.f32((int64_t)B * Ho * Co * Wo);
    if (blk.has_sc) {
      float* S = c.a.f32((int64_t)B * H * Co * W);
      for (int b = 0; b < B; ++b) conv(c, e, rows(P, b, H, C, W, 1, 1), blk.wsc, plain(S, b, H, Co, W), ConvOpt());
      RUN(c, g_be.avgpool2x2(S, (int64_t)H * Co * W, (int64_t)Co * W, W, B, Co, H, W, SC, (int64_t)Ho * Co * Wo, (int64_t)Co * Wo,
                             Wo, c.stream));
    } else {
      RUN(c, g_be.avgpool2x2(P + (int64_t)C * W, (int64_t)(H + 2) * C * W, (int64_t)C * W, W, B, C, H, W, SC,
                             (int64_t)Ho * Co * Wo, (int64_t)Co * Wo, Wo, c.stream));
    }
    // residual: leaky -> conv1 3x3 -> depthwise stride-2 3x3 -> leaky -> conv2 3x3 (models.py:125-135)
    float* R1 = c.a.f32((int64_t)B * H * C * W);
    for (int b = 0; b < B; ++b) {
      ConvOpt o;
      o.pad_left = 1; o.bias = e.F(blk.b1); o.pro = ST2_PRO_LEAKY; o.slope = 0.2f;
      conv(c, e, rows(P, b, H, C, W, 3, 0), blk.w1, plain(R1, b, H, C, W), o);
    }
    float* P2 = new_map(Ho, C, Wo);
    RUN(c, g_be.dwconv3x3s2(R1, (int64_t)H * C * W, (int64_t)C * W, W, e.F(blk.wd), e.F(blk.bd), B, C, H, W, P2 + (int64_t)C * Wo,
                            (int64_t)(Ho + 2) * C * Wo, (int64_t)C * Wo, Wo, c.stream));
    float* Pn = new_map(Ho, Co, Wo);
    for (int b = 0; b < B; ++b) {  // (shortcut + residual) / sqrt(2) in the epilogue
      ConvOpt o;
      o.pad_left = 1; o.bias = e.F(blk.b2); o.pro = ST2_PRO_LEAKY; o.slope = 0.2f;
      o.res = plain(SC, b, Ho, Co, Wo); o.div = (float)sqrt(2.0);
      View y = rows(Pn, b, Ho, Co, Wo, 1, 1);
      conv(c, e, rows(P2, b, Ho, C, Wo, 3, 0), blk.w2, y, o);
    }
    P = Pn; H = Ho; W = Wo; C = Co;
  }
  // LeakyReLU -> 5x5 valid conv -> global average -> LeakyReLU -> Linear (models.py:151-163)
  const int Cl = s.c_last, Wf = W - 4;
  float* Fm = c.a.f32((int64_t)B * Cl * Wf);
  for (int b = 0; b < B; ++b) {
    View x;
    x.p = P + (int64_t)b * (H + 2) * C * W + (int64_t)C * W;
    x.B = 1; x.C = 5 * C; x.L = W; x.bs = (int64_t)5 * C * W; x.cs = W;
    View y;
    y.p = Fm + (int64_t)b * Cl * Wf;
    y.B = 1; y.C = Cl; y.L = Wf; y.bs = (int64_t)Cl * Wf; y.cs = Wf;
    ConvOpt o;
    o.bias = e.F(s.b5); o.pro = ST2_PRO_LEAKY; o.slope = 0.2f;
    conv(c, e, x, s.w5, y, o);
  }
  float* m = c.a.f32((int64_t)B * Cl);
  RUN(c, g_be.mean_tokens_len(Fm, (int64_t)Cl * Wf, Wf, m, Cl, B, Cl, Wf, nullptr, c.stream));
  {
    View x, y;
    x.p = m; x.B = B; x.C = Cl; x.L = 1; x.bs = Cl; x.cs = 1;
    y.p = out; y.B = B; y.C = s.style_dim; y.L = 1; y.bs = s.style_dim; y.cs = 1;
    ConvOpt o;
    o.bias = e.F(s.bl); o.pro = ST2_PRO_LEAKY; o.slope = 0.2f;
    conv(c, e, x, s.wl, y, o);
  }
  return c.rc;
}

// ------------------------------------------------------------------------------------------------------------------
// ragged style plan == style_plan on B clips of unequal width in one [B][H][W] buffer (W = the capacity), row b as the clip
// alone: every Conv2d ONE launch over the B (h + 2) - 2 stacked rows of the padded maps.  Three consecutive padded rows are a
// conv's input channels whichever clip they belong to; a stacked row whose centre is an image row of clip b gets
// x_len = y_len = that clip's width, one whose centre is a zero row between two clips (a seam) gets 0: its tiles exit before
// any barrier and store nothing, so the zero rows stay zero.  Buffers the uniform plan keeps unpadded (S, R1, SC) take the
// padded row stride here, so that one base pointer and one row stride describe the whole batch.
// ------------------------------------------------------------------------------------------------------------------
int style_plan_ragged(Ctx& c, const st2_engine& e, const PStyleEnc& s, const float* mel, const int32_t* mel_len, int B, int H,
                      int W, float* out) {
  constexpr int S = 4;  // down-sampling stages (pack_style checks the block count)
  // length tables (st2.h st2_style_lengths): per clip W_0 .. W_4 and W_4 - 4, then one per-stacked-row table per stage
  const int64_t n_tab = st2_style_lengths_count(B, H, S);
  int32_t* tab = static_cast<int32_t*>(c.a.alloc(n_tab * 4));
  RUN(c, g_be.style_lengths(mel_len, B, 80, W, H, S, tab, c.stream));
  const int32_t* wlen[S + 2];
  const int32_t* rlen[S + 1];
  for (int i = 0; i < S + 2; ++i) wlen[i] = tab + (int64_t)i * B;
  {
    int64_t off = (int64_t)(S + 2) * B;
    for (int i = 0; i <= S; ++i) {
      rlen[i] = tab + off;
      off += (int64_t)B * ((H >> i) + 2) - 2;
    }
  }
  auto new_map = [&](int h, int ch, int w) -> float* {  // as in style_plan: rows 0 and h + 1 of every clip are zero
    float* p = c.a.f32((int64_t)B * (h + 2) * ch * w);
    for (int r : {0, h + 1})
      RUN(c, g_be.broadcast_cols(e.F(e.zeros), 0, p + (int64_t)r * ch * w, (int64_t)(h + 2) * ch * w, w, B, ch, w, c.stream));
    return p;
  };
  // padded rows r0 + r .. r0 + r + k - 1 of the whole [B (h + 2)][ch][w] stack as the channels of stacked row r:
  // k = 3 from row 0 (a 3x3 conv's input) and k = 1 from row 1 (its output, a 1x1 conv's input) have the same centre row r + 1
  auto stack = [&](float* P, int h, int ch, int w, int k, int r0, const int32_t* len) {
    View v;
    v.p = P + (int64_t)r0 * ch * w;
    v.B = B * (h + 2) - 2; v.C = k * ch; v.L = w; v.bs = (int64_t)ch * w; v.cs = w; v.len = len;
    return v;
  };
  float* m0 = new_map(H, 1, W);
  RUN(c, g_be.copy_ncl(mel, (int64_t)H * W, W, m0 + W, (int64_t)(H + 2) * W, W, B, H, W, c.stream));
  int C = s.c0;
  float* P = new_map(H, C, W);
  {
    const View x = stack(m0, H, 1, W, 3, 0, rlen[0]);
    RUN(c, g_be.conv1d_direct_len(x.p, x.bs, x.cs, e.F(s.w0), e.F(s.b0), P + (int64_t)C * W, (int64_t)C * W, W, x.B, 3, C, W, W, 3,
                                  1, 1, rlen[0], rlen[0], c.stream));
  }
  int st = 0;
  for (const PStyleBlk& blk : s.blocks) {
    const int Co = blk.c_out, Ho = H / 2, Wo = (W + 1) / 2;
    const int32_t* rl = rlen[st];
    const int32_t* rlo = rlen[st + 1];
    // shortcut: 1x1 conv at full resolution, then the 2x2 average (models.py:118-123)
    float* SC = c.a.f32((int64_t)B * (Ho + 2) * Co * Wo);
    if (blk.has_sc) {
      float* Sm = c.a.f32((int64_t)B * (H + 2) * Co * W);
      ConvOpt o;
      o.split_rows = H;
      conv(c, e, stack(P, H, C, W, 1, 1, rl), blk.wsc, stack(Sm, H, Co, W, 1, 1, rl), o);
      RUN(c, g_be.avgpool2x2_len(Sm + (int64_t)Co * W, (int64_t)(H + 2) * Co * W, (int64_t)Co * W, W, B, Co, H, W,
                                 SC + (int64_t)Co * Wo, (int64_t)(Ho + 2) * Co * Wo, (int64_t)Co * Wo, Wo, wlen[st], c.stream));
    } else {
      RUN(c, g_be.avgpool2x2_len(P + (int64_t)C * W, (int64_t)(H + 2) * C * W, (int64_t)C * W, W, B, C, H, W,
                                 SC + (int64_t)Co * Wo, (int64_t)(Ho + 2) * Co * Wo, (int64_t)Co * Wo, Wo, wlen[st], c.stream));
    }
    // residual: leaky -> conv1 3x3 -> depthwise stride-2 3x3 -> leaky -> conv2 3x3 (models.py:125-135)
    float* R1 = c.a.f32((int64_t)B * (H + 2) * C * W);
    {
      ConvOpt o;
      o.pad_left = 1; o.bias = e.F(blk.b1); o.pro = ST2_PRO_LEAKY; o.slope = 0.2f; o.split_rows = H;
      conv(c, e, stack(P, H, C, W, 3, 0, rl), blk.w1, stack(R1, H, C, W, 1, 1, rl), o);
    }
    float* P2 = new_map(Ho, C, Wo);
    RUN(c, g_be.dwconv3x3s2_len(R1 + (int64_t)C * W, (int64_t)(H + 2) * C * W, (int64_t)C * W, W, e.F(blk.wd), e.F(blk.bd), B, C, H,
                                W, P2 + (int64_t)C * Wo, (int64_t)(Ho + 2) * C * Wo, (int64_t)C * Wo, Wo, wlen[st], c.stream));
    float* Pn = new_map(Ho, Co, Wo);
    {  // (shortcut + residual) / sqrt(2) in the epilogue
      ConvOpt o;
      o.pad_left = 1; o.bias = e.F(blk.b2); o.pro = ST2_PRO_LEAKY; o.slope = 0.2f; o.split_rows = Ho;
      o.res = stack(SC, Ho, Co, Wo, 1, 1, nullptr); o.div = (float)sqrt(2.0);
      conv(c, e, stack(P2, Ho, C, Wo, 3, 0, rlo), blk.w2, stack(Pn, Ho, Co, Wo, 1, 1, rlo), o);
    }
    P = Pn; H = Ho; W = Wo; C = Co;
    ++st;
  }
  // LeakyReLU -> 5x5 valid conv -> global average over the clip's own W_4 - 4 columns -> LeakyReLU -> Linear (models.py:151-163)
  const int Cl = s.c_last, Wf = W - 4;
  float* Fm = c.a.f32((int64_t)B * Cl * Wf);
  {
    View x;
    x.p = P + (int64_t)C * W;
    x.B = B; x.C = 5 * C; x.L = W; x.bs = (int64_t)(H + 2) * C * W; x.cs = W; x.len = wlen[S];
    View y;
    y.p = Fm;
    y.B = B; y.C = Cl; y.L = Wf; y.bs = (int64_t)Cl * Wf; y.cs = Wf; y.len = wlen[S + 1];
    ConvOpt o;
    o.bias = e.F(s.b5); o.pro = ST2_PRO_LEAKY; o.slope = 0.2f; o.split_rows = 1;
    conv(c, e, x, s.w5, y, o);
  }
  float* m = c.a.f32((int64_t)B * Cl);
  RUN(c, g_be.mean_tokens_len(Fm, (int64_t)Cl * Wf, Wf, m, Cl, B, Cl, Wf, wlen[S + 1], c.stream));
  {
    View x, y;
    x.p = m; x.B = B; x.C = Cl; x.L = 1; x.bs = Cl; x.cs = 1;
    y.p = out; y.B = B; y.C = s.style_dim; y.L = 1; y.bs = s.style_dim; y.cs = 1;
    ConvOpt o;
    o.bias = e.F(s.bl); o.pro = ST2_PRO_LEAKY; o.slope = 0.2f;
    conv(c, e, x, s.wl, y, o);
  }
  return c.rc;
}

bool check_cfg(const st2_model_config& c) {
  return c.n_upsamples >= 1 && c.n_upsamples <= 4 && c.n_resblock_kernels >= 1 && c.n_resblock_kernels <= 4 &&
         (c.decoder_kind == 0 || c.decoder_kind == 1) && c.dim_in > 0 && c.style_dim > 0 && c.dn_layers >= 0;
}
