// Launch plan: PL-BERT and the one-call front (text encoder, PL-BERT, sampler, style mixing, duration stages).  Textually included by st2_engine.hip INSIDE its anonymous namespace (one translation unit:
// the plans share the packed-weight structs, the workspace arena and conv() defined there); split out per plan in round 6.

// ------------------------------------------------------------------------------------------------------------------
// PL-BERT plan == CustomAlbert.forward_engine (styletts2_amd/text.py); front plan == pipeline._front_core
// ------------------------------------------------------------------------------------------------------------------
int pack_bert(st2_engine& e, Blob& blob, std::string* err) {
  Packer pk{e, blob};
  PBert b;
  const std::string R = "bert.", L = R + "encoder.albert_layer_groups.0.albert_layers.0.";
  const HostTensor* w = pk.get(R + "embeddings.word_embeddings.weight");
  const HostTensor* p = pk.get(R + "embeddings.position_embeddings.weight");
  const HostTensor* tt = pk.get(R + "embeddings.token_type_embeddings.weight");
  const HostTensor* q = pk.get(L + "attention.query.weight");
  const HostTensor* k = pk.get(L + "attention.key.weight");
  const HostTensor* v = pk.get(L + "attention.value.weight");
  const HostTensor* qb = pk.get(L + "attention.query.bias");
  const HostTensor* kb = pk.get(L + "attention.key.bias");
  const HostTensor* vb = pk.get(L + "attention.value.bias");
  if (!pk.ok || w->shape.size() != 2 || p->shape.size() != 2 || tt->shape.size() != 2 || q->shape.size() != 2) {
    *err = "PL-BERT parameter missing or malformed: " + pk.missing;
    return 1;
  }
  b.V = (int)w->shape[0]; b.E = (int)w->shape[1]; b.P = (int)p->shape[0]; b.H = (int)q->shape[0];
  if (p->shape[1] != b.E || tt->shape[1] != b.E || q->shape[1] != b.H || k->numel() != q->numel() ||
      v->numel() != q->numel() || qb->numel() != b.H || kb->numel() != b.H || vb->numel() != b.H || b.H % 64 != 0 ||
      e.cfg.bert_layers <= 0) {
    *err = "PL-BERT: inconsistent shapes (64-wide heads, one shared layer) or cfg.bert_layers == 0";
    return 1;
  }
  b.word = blob.add_f32(w->data);
  b.pos = blob.add_f32(p->data);
  b.tok0 = blob.add_f32(std::vector<float>(tt->data.begin(), tt->data.begin() + b.E));  // token_type_ids == 0 everywhere
  b.eln_w = pk.vec(R + "embeddings.LayerNorm.weight", b.E); b.eln_b = pk.vec(R + "embeddings.LayerNorm.bias", b.E);
  b.map = pk.conv_w(R + "encoder.embedding_hidden_mapping_in.weight", b.H, b.E, 1);
  b.map_b = pk.vec(R + "encoder.embedding_hidden_mapping_in.bias", b.H);
  {  // q | k | v as one 3H-row Linear
    const size_t HH = (size_t)b.H * b.H;
    std::vector<float> cat(3 * HH), bias((size_t)3 * b.H);
    std::copy(q->data.begin(), q->data.end(), cat.begin());
    std::copy(k->data.begin(), k->data.end(), cat.begin() + HH);
    std::copy(v->data.begin(), v->data.end(), cat.begin() + 2 * HH);
    std::copy(qb->data.begin(), qb->data.end(), bias.begin());
    std::copy(kb->data.begin(), kb->data.end(), bias.begin() + b.H);
    std::copy(vb->data.begin(), vb->data.end(), bias.begin() + 2 * b.H);
    b.qkv = pack_split(blob, L + "attention.query|key|value.weight", cat.data(), 3 * b.H, b.H, 1);
    b.qkv_b = blob.add_f32(bias);
  }
  b.dense = pk.conv_w(L + "attention.dense.weight", b.H, b.H, 1); b.dense_b = pk.vec(L + "attention.dense.bias", b.H);
  b.aln_w = pk.vec(L + "attention.LayerNorm.weight", b.H);        b.aln_b = pk.vec(L + "attention.LayerNorm.bias", b.H);
  b.ffn = pk.conv_w(L + "ffn.weight", -1, b.H, 1);
  b.I = b.ffn.C_out;
  b.ffn_b = pk.vec(L + "ffn.bias", b.I > 0 ? b.I : -1);
  b.out = pk.conv_w(L + "ffn_output.weight", b.H, b.I > 0 ? b.I : -1, 1); b.out_b = pk.vec(L + "ffn_output.bias", b.H);
  b.fln_w = pk.vec(L + "full_layer_layer_norm.weight", b.H);      b.fln_b = pk.vec(L + "full_layer_layer_norm.bias", b.H);
  if (pk.has("bert_encoder.weight")) {
    b.enc = pk.conv_w("bert_encoder.weight", -1, b.H, 1);
    b.enc_b = pk.vec("bert_encoder.bias", b.enc.C_out > 0 ? b.enc.C_out : -1);
    b.has_enc = true;
  }
  if (!pk.ok) { *err = "PL-BERT parameter missing or malformed: " + pk.missing; return 1; }
  b.ready = true;
  e.bert = b;
  return 0;
}

// -> the last hidden state as a [B][H][N] view of token-merged storage ([H][B*N]); lives in the arena
View bert_plan(Ctx& c, const st2_engine& e, const int64_t* tokens, const int32_t* lens, int B, int N) {
  const PBert& p = e.bert;
  const float eps = e.cfg.bert_ln_eps;
  const int H = p.H, heads = H / 64;
  Sess s{c, e, B, N, true, lens, {}, 0, nullptr, nullptr, 1.0};
  View X = dn_alloc(s, H), Xn = dn_alloc(s, H);
  {
    const int64_t mark = c.a.off;
    View E = dn_alloc(s, p.E);
    RUN(c, g_be.embed_tokens(tokens, B, N, e.F(p.word), p.V, p.E, e.F(p.tok0), e.F(p.pos), nullptr, E.p, E.bs, E.cs,
                             c.stream));
    float* st = c.a.f32((int64_t)B * N * 2);
    RUN(c, g_be.colnorm_stats(E.p, E.bs, E.cs, B, p.E, N, eps, st, c.stream));
    ConvOpt o;  // embedding LayerNorm in the prologue of the E -> H mapping
    o.bias = e.F(p.map_b); o.pro = ST2_PRO_COLNORM; o.stats = st; o.gamma = e.F(p.eln_w); o.beta = e.F(p.eln_b);
    conv(c, e, dn_cv(s, E), p.map, dn_cv(s, X), o);
    c.a.off = mark;
  }
  for (int l = 0; l < e.cfg.bert_layers; ++l) {
    const int64_t mark = c.a.off;
    View qkv = dn_alloc(s, 3 * H);
    {
      ConvOpt o;
      o.bias = e.F(p.qkv_b);
      conv(c, e, dn_cv(s, X), p.qkv, dn_cv(s, qkv), o);
    }
    View ctx = dn_alloc(s, H);
    View q = qkv.rows(0, H), k = qkv.rows(H, 2 * H), v = qkv.rows(2 * H, 3 * H);
    RUN(c, g_be.attention_keylen(q.p, k.p, v.p, q.bs, q.cs, ctx.p, ctx.bs, ctx.cs, B, heads, 64, N, 0.125f, lens, c.stream));
    View Y = dn_alloc(s, H);
    {
      ConvOpt o;
      o.bias = e.F(p.dense_b); o.res = dn_cv(s, X);
      conv(c, e, dn_cv(s, ctx), p.dense, dn_cv(s, Y), o);
    }
    float* st1 = c.a.f32((int64_t)B * N * 2);
    RUN(c, g_be.colnorm_stats(Y.p, Y.bs, Y.cs, B, H, N, eps, st1, c.stream));
    View X1 = dn_alloc(s, H);
    RUN(c, g_be.colnorm_apply(Y.p, Y.bs, Y.cs, st1, e.F(p.aln_w), e.F(p.aln_b), 0, 0, ST2_ACT_NONE, 0.f, nullptr, X1.p, X1.bs,
                              X1.cs, B, H, N, c.stream));
    View Hm = dn_alloc(s, p.I);
    {
      ConvOpt o;
      o.bias = e.F(p.ffn_b); o.act = ST2_ACT_GELU_TANH;
      conv(c, e, dn_cv(s, X1), p.ffn, dn_cv(s, Hm), o);
    }
    View Z = dn_alloc(s, H);
    {
      ConvOpt o;
      o.bias = e.F(p.out_b); o.res = dn_cv(s, X1);
      conv(c, e, dn_cv(s, Hm), p.out, dn_cv(s, Z), o);
    }
    float* st2 = c.a.f32((int64_t)B * N * 2);
    RUN(c, g_be.colnorm_stats(Z.p, Z.bs, Z.cs, B, H, N, eps, st2, c.stream));
    RUN(c, g_be.colnorm_apply(Z.p, Z.bs, Z.cs, st2, e.F(p.fln_w), e.F(p.fln_b), 0, 0, ST2_ACT_NONE, 0.f, nullptr, Xn.p, Xn.bs,
                              Xn.cs, B, H, N, c.stream));
    std::swap(X, Xn);
    c.a.off = mark;
  }
  return X;
}

int front_plan(Ctx& c, const st2_engine& e, const st2_front_args& a, const st2_controls* ctl = nullptr,
               const float* tok_speed = nullptr) {
  const st2_model_config& cfg = e.cfg;
  const int B = a.B, N = a.N, sty = cfg.style_dim, C2 = cfg.dn_channels, dh = cfg.pred_hidden;
  text_plan(c, e, a.tokens, a.lengths, B, N, a.t_en);
  View X = bert_plan(c, e, a.tokens, a.lengths, B, N);
  Sess s0{c, e, B, N, true, a.lengths, {}, 0, nullptr, nullptr, 1.0};
  View D = dn_alloc(s0, dh);  // bert_encoder: Linear(H -> hidden_dim) over the merged tokens == d_en channel-major
  {
    ConvOpt o;
    o.bias = e.F(e.bert.enc_b);
    conv(c, e, dn_cv(s0, X), e.bert.enc, dn_cv(s0, D), o);
  }
  const int64_t n = (int64_t)B * C2;
  float* sp = c.a.f32(n);
  {
    const int64_t mark = c.a.off;
    if (sampler_plan(c, e, a.noise, nullptr, &X, a.ref_s, a.step_noise, a.lengths, B, N, a.steps, a.embedding_scale, a.table,
                     a.sigma0, sp, nullptr) != 0 && c.rc == 0)
      c.rc = 1;
    c.a.off = mark;
  }
  const float* speed = ctl ? ctl->speed : nullptr;
  if (ctl && (ctl->alpha || ctl->beta || ctl->t)) {
    // per-row weights: the whole mixing -- in carry mode the row scan too -- is ONE launch (st2_controls.hip), the arithmetic of
    // the launches below in their order
    RUN(c, st2_style_mix_rows(sp, a.s_prev, a.ref_s, ctl->t, ctl->alpha, ctl->beta, a.t, a.alpha, a.beta, B, sty,
                              a.carry && B > 1, a.ref, a.s, a.s_pred_out, c.stream));
    duration_plan(c, e, D, a.s, a.lengths, B, N, a.tail, a.d_cm, a.durations, speed, tok_speed);
    return c.rc;
  }
  if (a.carry && B > 1) {
    // the rows are consecutive sentences of one passage: row k mixes with row k-1's MIXED style (the loop of LFinference,
    // Demo/Inference_LibriTTS.ipynb LFinference: `s_prev = s_pred` after the speaker mixing).  A scan of the same elementwise
    // launches the one-sentence call makes, on one row each: bitwise the sentence-by-sentence results, ~5 us per launch.
    float* mixed = a.s_pred_out ? a.s_pred_out : c.a.f32(n);
    float* m = c.a.f32(C2);
    float* ma = c.a.f32(C2);
    float* mb = c.a.f32(C2);
    for (int k = 0; k < B; ++k) {
      const float* prev = k ? mixed + (int64_t)(k - 1) * C2 : a.s_prev;
      const float* cur = sp + (int64_t)k * C2;
      if (prev) {
        RUN(c, g_be.axpbypcz(prev, (float)a.t, cur, (float)(1.0 - a.t), nullptr, 0.f, m, C2, c.stream));
        cur = m;
      }
      const float* ref_src = cur;
      const float* s_src = cur + sty;
      if (a.ref_s) {
        const float* rs = a.ref_s + (int64_t)k * C2;
        RUN(c, g_be.axpbypcz(cur, (float)a.alpha, rs, (float)(1.0 - a.alpha), nullptr, 0.f, ma, C2, c.stream));
        RUN(c, g_be.axpbypcz(cur, (float)a.beta, rs, (float)(1.0 - a.beta), nullptr, 0.f, mb, C2, c.stream));
        ref_src = ma;
        s_src = mb + sty;
      }
      RUN(c, g_be.copy_ncl(ref_src, C2, sty, mixed + (int64_t)k * C2, C2, sty, 1, 1, sty, c.stream));
      RUN(c, g_be.copy_ncl(s_src, C2, sty, mixed + (int64_t)k * C2 + sty, C2, sty, 1, 1, sty, c.stream));
    }
    RUN(c, g_be.copy_ncl(mixed, C2, sty, a.ref, sty, sty, B, 1, sty, c.stream));
    RUN(c, g_be.copy_ncl(mixed + sty, C2, sty, a.s, sty, sty, B, 1, sty, c.stream));
    duration_plan(c, e, D, a.s, a.lengths, B, N, a.tail, a.d_cm, a.durations, speed, tok_speed);
    return c.rc;
  }
  const float* cur = sp;
  if (a.s_prev) {  // LFinference: convex combination of the previous and the current style
    float* m = c.a.f32(n);
    RUN(c, g_be.axpbypcz(a.s_prev, (float)a.t, cur, (float)(1.0 - a.t), nullptr, 0.f, m, n, c.stream));
    cur = m;
  }
  const float* ref_src = cur;
  const float* s_src = cur + sty;
  if (a.ref_s) {  // Demo/Inference_LibriTTS.ipynb:289-290
    float* ma = c.a.f32(n);
    float* mb = c.a.f32(n);
    RUN(c, g_be.axpbypcz(cur, (float)a.alpha, a.ref_s, (float)(1.0 - a.alpha), nullptr, 0.f, ma, n, c.stream));
    RUN(c, g_be.axpbypcz(cur, (float)a.beta, a.ref_s, (float)(1.0 - a.beta), nullptr, 0.f, mb, n, c.stream));
    ref_src = ma;
    s_src = mb + sty;
  }
  RUN(c, g_be.copy_ncl(ref_src, C2, sty, a.ref, sty, sty, B, 1, sty, c.stream));
  RUN(c, g_be.copy_ncl(s_src, C2, sty, a.s, sty, sty, B, 1, sty, c.stream));
  if (a.s_pred_out) {
    RUN(c, g_be.copy_ncl(ref_src, C2, sty, a.s_pred_out, C2, sty, B, 1, sty, c.stream));
    RUN(c, g_be.copy_ncl(s_src, C2, sty, a.s_pred_out + sty, C2, sty, B, 1, sty, c.stream));
  }
  duration_plan(c, e, D, a.s, a.lengths, B, N, a.tail, a.d_cm, a.durations, speed, tok_speed);
  return c.rc;
}
