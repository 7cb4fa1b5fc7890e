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

// One 2-D feature map of the plan, [B][h (+ 2)][ch][w]: p is row 1 of a padded map (image row 0 of clip 0) or the start of an
// unpadded one, bs the stride between clips.
struct StyleMap {
  float* p = nullptr;
  int64_t bs = 0;
  int h = 0, ch = 0, w = 0;
  int64_t row() const { return (int64_t)ch * w; }
};

// Uniform batch (mel_len == NULL): every Conv2d once per clip, on the h image rows of that clip; the buffers that are no conv's
// 3-row input (the shortcut before and after its pool, conv1's output) are unpadded [B][h][ch][w].  Plain backend slots only.
//
// Ragged batch (mel_len: int32 [B] frame counts on the device; W = the capacity), row b as the clip alone: every Conv2d ONE
// launch over the B (h + 2) - 2 stacked rows of the padded maps.  Three consecutive padded rows are a conv's input channels
// whichever clip they belong to; a stacked row whose centre is an image row of clip b gets x_len = y_len = that clip's width,
// one whose centre is a zero row between two clips (a seam) gets 0: its tiles exit before any barrier and store nothing, so the
// zero rows stay zero.  Every buffer takes the padded row stride, so that one base pointer and one row stride describe the whole
// batch; the map kernels get the clips' widths.  A dry walk reads no lengths: any non-null mel_len selects this layout.
int style_plan(Ctx& c, const st2_engine& e, const PStyleEnc& s, const float* mel, const int32_t* mel_len, int B, int H, int W,
               float* out) {
  constexpr int S = 4;  // down-sampling stages (pack_style checks the block count)
  const bool ragged = mel_len != nullptr;
  // ragged only -- length tables (st2.h st2_style_lengths): per clip W_0 .. W_4 and W_4 - 4, then one per-stacked-row table per stage
  const int32_t* wlen[S + 2] = {};
  const int32_t* rlen[S + 1] = {};
  if (ragged) {
    int32_t* tab = static_cast<int32_t*>(c.a.alloc(st2_style_lengths_count(B, H, S) * 4));
    RUN(c, g_be.style_lengths(mel_len, B, 80, W, H, S, tab, c.stream));
    for (int i = 0; i < S + 2; ++i) wlen[i] = tab + (int64_t)i * B;
    int64_t off = (int64_t)(S + 2) * B;
    for (int i = 0; i <= S; ++i) {
      rlen[i] = tab + off;
      off += (int64_t)B * ((H >> i) + 2) - 2;
    }
  }
  // a map whose rows 0 and h + 1 are zero in every clip (the rows 1 .. h are written by the producing kernel): a 3x3 conv's input
  auto new_map = [&](int h, int ch, int w) {
    StyleMap m{c.a.f32((int64_t)B * (h + 2) * ch * w), (int64_t)(h + 2) * ch * w, h, ch, w};
    for (int r : {0, h + 1}) RUN(c, g_be.broadcast_cols(e.F(e.zeros), 0, m.p + r * m.row(), m.bs, w, B, ch, w, c.stream));
    m.p += m.row();
    return m;
  };
  // a map that is never a 3x3 conv's input: unpadded, or (ragged) padded like the others with its outer rows left unwritten
  auto scratch = [&](int h, int ch, int w) {
    const int pad = ragged ? 2 : 0;
    StyleMap m{c.a.f32((int64_t)B * (h + pad) * ch * w), (int64_t)(h + pad) * ch * w, h, ch, w};
    m.p += (pad / 2) * m.row();
    return m;
  };
  // k rows around each row of m stacked along the channels (k = 3: a 3x3 conv's input, from the row above; k = 1: the row
  // itself): [h][k ch][w] of clip b (overlapping view), or (ragged, len = the stage's row table) of the whole stack
  auto rows = [&](const StyleMap& m, int k, int b, const int32_t* len) {
    View v;
    v.p = m.p - (k / 2) * m.row() + (ragged ? 0 : b * m.bs);
    v.B = ragged ? B * (m.h + 2) - 2 : m.h;
    v.C = k * m.ch; v.L = m.w; v.bs = m.row(); v.cs = m.w; v.len = len;
    return v;
  };
  const int launches = ragged ? 1 : B;  // per Conv2d
  // the Conv2d wt over all clips: k stacked rows of x -> y, res (optional) added in the epilogue
  auto conv2d = [&](const StyleMap& x, int k, const SplitW& wt, const StyleMap& y, ConvOpt o, const StyleMap* res,
                    const int32_t* len) {
    o.split_rows = ragged ? x.h : 0;
    for (int b = 0; b < launches; ++b) {
      if (res) o.res = rows(*res, 1, b, nullptr);
      conv(c, e, rows(x, k, b, len), wt, rows(y, 1, b, len), o);
    }
  };
  StyleMap m0 = new_map(H, 1, W);
  RUN(c, g_be.copy_ncl(mel, (int64_t)H * W, W, m0.p, m0.bs, W, B, H, W, c.stream));
  StyleMap P = new_map(H, s.c0, W);
  for (int b = 0; b < launches; ++b)
    conv1d_direct(c, rows(m0, 3, b, rlen[0]), e.F(s.w0), e.F(s.b0), rows(P, 1, b, rlen[0]), 3, 1, 1);
  int st = 0;
  for (const PStyleBlk& blk : s.blocks) {
    const int C = P.ch, Co = blk.c_out, Ho = P.h / 2, Wo = (P.w + 1) / 2;
    ConvOpt leaky;  // every 3x3 conv of the block: LeakyReLU on its input, zero column padding, bias
    leaky.pad_left = 1; leaky.pro = ST2_PRO_LEAKY; leaky.slope = 0.2f;
    // shortcut: 1x1 conv at full resolution, then the 2x2 average (models.py:118-123)
    StyleMap SC = scratch(Ho, Co, Wo);
    StyleMap Sm = P;
    if (blk.has_sc) {
      Sm = scratch(P.h, Co, P.w);
      conv2d(P, 1, blk.wsc, Sm, ConvOpt(), nullptr, rlen[st]);
    }
    avgpool2x2(c, Sm.p, Sm.bs, Sm.row(), Sm.w, B, Sm.ch, Sm.h, Sm.w, SC.p, SC.bs, SC.row(), Wo, wlen[st]);
    // residual: leaky -> conv1 3x3 -> depthwise stride-2 3x3 -> leaky -> conv2 3x3 (models.py:125-135)
    StyleMap R1 = scratch(P.h, C, P.w);
    leaky.bias = e.F(blk.b1);
    conv2d(P, 3, blk.w1, R1, leaky, nullptr, rlen[st]);
    StyleMap P2 = new_map(Ho, C, Wo);
    dwconv3x3s2(c, R1.p, R1.bs, R1.row(), R1.w, e.F(blk.wd), e.F(blk.bd), B, C, R1.h, R1.w, P2.p, P2.bs, P2.row(), Wo, wlen[st]);
    StyleMap Pn = new_map(Ho, Co, Wo);
    leaky.bias = e.F(blk.b2); leaky.div = (float)sqrt(2.0);  // (shortcut + residual) / sqrt(2) in the epilogue
    conv2d(P2, 3, blk.w2, Pn, leaky, &SC, rlen[st + 1]);
    P = Pn;
    ++st;
  }
  // LeakyReLU -> 5x5 valid conv (the 5 image rows as its channels) -> global average (ragged: over the clip's own W_4 - 4
  // columns) -> LeakyReLU -> Linear (models.py:151-163)
  const int Cl = s.c_last, Wf = P.w - 4;
  float* Fm = c.a.f32((int64_t)B * Cl * Wf);
  for (int b = 0; b < launches; ++b) {
    const int nb = ragged ? B : 1;  // clips of this launch
    View x, y;
    x.p = P.p + b * P.bs; x.B = nb; x.C = 5 * P.ch; x.L = P.w; x.bs = ragged ? P.bs : 5 * P.row(); x.cs = P.w; x.len = wlen[S];
    y.p = Fm + (int64_t)b * Cl * Wf; y.B = nb; y.C = Cl; y.L = Wf; y.bs = (int64_t)Cl * Wf; y.cs = Wf; y.len = wlen[S + 1];
    ConvOpt o;
    o.bias = e.F(s.b5); o.pro = ST2_PRO_LEAKY; o.slope = 0.2f; o.split_rows = ragged ? 1 : 0;
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
