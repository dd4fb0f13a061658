// Included by decoder.hip inside its anonymous namespace: the tape (the placement table of a training forward, which keeps every
// tensor the backward needs) and the backward pass of `GradLogPEstimator2d` (reference: autograd through unitspeech/unitspeech.py:164-201,
// driven by `loss.backward()` at finetune.py:163).  Gradient conventions:
//   * a tensor that is stored pre-multiplied by the frame mask has a gradient that is masked too (its producer's
//     backward would multiply by the mask anyway), so data-gradient GEMMs of such tensors apply the mask in their epilogue;
//   * the attention reads its input raw, so the gradient w.r.t. a ResnetBlock output feeding attention is unmasked.

// zero-fill with a kernel of this library: ordered on the stream exactly like the launches around it
inline hipError_t zero_f32(float* p, size_t n, hipStream_t s) {
  while (n > 0) {
    const size_t chunk = n > (size_t)1 << 30 ? (size_t)1 << 30 : n;
    hipError_t e = launch_fill(p, 0.f, (int)chunk, s);
    if (e != hipSuccess) return e;
    p += chunk;
    n -= chunk;
  }
  return hipSuccess;
}
inline hipError_t zero_f64(double* p, size_t n, hipStream_t s) { return zero_f32(reinterpret_cast<float*>(p), 2 * n, s); }

// The placement table of a training step, every entry a slot of its own that lives until the backward, and the backward's scratch
struct Tape : Places {
  int Bp = 0, T = 0;
  bool forward_done = false;
  const float* mask = nullptr; int Bm = 0;   // library-owned copy inside the workspace (the caller's tensor may be gone by backward)
  float* mask_copy = nullptr;
  Buffers fb;                       // forward scratch that is not saved per layer (time embedding, attention partials, in2)
  // backward scratch
  std::vector<float*> GA, GB, GY, GY2, GH, GQKV, GO, GCAT;
  // scratch of the parameter-gradient chains, one set per side stream of the backward pass (BwdCtx): packed weight gradient, the
  // attention's M1 = G^T q and column sums
  static constexpr int kSideMax = 3;
  float *wscratch[kSideMax] = {}, *M1[kSideMax] = {}, *colsumG[kSideMax] = {};
  float *weff_dg = nullptr, *gctx = nullptr, *gtproj = nullptr, *gtemb = nullptr, *gmlp_h = nullptr;
  size_t gctx_stride = 0;           // floats between the gctx blocks of consecutive attention blocks (execution order of `att`)
  float* zero_lo = nullptr;         // [zero_lo, zero_lo + zero_floats): gsum, gctx, gtproj, gtemb, gmlp_h, amax -- zeroed by one fill per backward
  size_t zero_floats = 0;
  double* gsum = nullptr;           // one [B][8][2] block per GroupNorm backward, zeroed together
  int gsum_next = 0;
  size_t wscratch_floats = 0;
  // optional input gradients of the current backward call (caller-owned, planar [Bp][F][T] / [Bp][S]; null = not wanted)
  float *grad_x = nullptr, *grad_mu = nullptr, *grad_spk = nullptr;
  float* gscaled = nullptr;         // grad_out times the power of two us_estimator_backward picks ([Bp][F][T])
  const float* unscale = nullptr;   // device scalar 2^-k of the current backward call (null: no loss scaling, exact-fp32 handle)
  double* red_partials = nullptr;   // fp64 partial sums of the scalar gradients: kRedBlocks per attention (execution order), then the final bias's
  float* amax = nullptr;            // one word per weight-gradient launch of a backward pass: max |gy| (launch_wgrad_amax), zeroed together
  int amax_next = 0;
  static constexpr int kAmaxSlots = 256;
};

inline void plan_train(us_decoder* h, Arena& A, int Bp, int T, Tape& tp) {
  const int L = h->cfg.n_mults, F = h->cfg.n_feats;
  const size_t B = (size_t)Bp;
  tp.Bp = Bp; tp.T = T;
  // of the forward's scratch only what no layer keeps; the backward reads fb.in2 / posemb / mlp_h / temb / tproj_off and runs its
  // convolutions through fb.splitk and fb.wino_v / wino_m
  plan_shared(h, A, Bp, T, tp.fb, true);
  init_places(h, A, Bp, tp);
  auto npx = [&](int l) { return (size_t)(F >> l) * (T >> l); };
  for (int l = 1; l < L; ++l) tp.CAT[l] = A.alloc<float>(B * npx(l) * 2 * h->C[l]);
  // out: null = a slot of its own, `ld` wide
  auto plan_res = [&](const ResnetW& r, float* out, int ld) {
    ResT& t = tp.res[r.index];
    const size_t n = npx(r.level);
    t.y1 = A.alloc<float>(B * n * r.cout);
    t.h1 = A.alloc<float>(B * n * r.cout);
    t.y2 = A.alloc<float>(B * n * r.cout);
    if (r.first) t.r0 = A.alloc<float>(B * n * r.cout);
    t.out = out ? out : A.alloc<float>(B * n * ld); t.out_ld = ld;
  };
  auto plan_att = [&](AttT& t, float* out, int ld) {
    const size_t n = npx(t.w->level);
    t.qkv = A.alloc<float>(B * n * 3 * kHidden);
    t.ctx = A.alloc<float>(B * kHeads * kDimHead * kDimHead);
    t.colM = A.alloc<float>(B * kHidden);
    t.colS = A.alloc<float>(B * kHidden);
    t.weff = A.alloc<float>(B * (size_t)t.w->dim * kHidden);
    t.o_pre = A.alloc<float>(B * n * (size_t)t.w->dim);
    t.out = out ? out : A.alloc<float>(B * n * ld); t.out_ld = ld;
  };
  for (int l = 0; l < L; ++l) {
    auto& d = h->downs[l];
    const int c = h->C[l];
    plan_res(d.r1, nullptr, c); plan_res(d.r2, nullptr, c);
    if (l == 0) plan_att(tp.att[0], nullptr, c);
    else plan_att(tp.att[l], tp.CAT[l] + c, 2 * c);
    if (d.has_ds) { tp.downs[l].out = A.alloc<float>(B * npx(l + 1) * c); tp.downs[l].out_ld = c; }
  }
  const int lm = L - 1, cm = h->C[lm];
  plan_res(h->mid1, nullptr, cm);
  plan_att(tp.att[L], nullptr, cm);
  if (L > 1) plan_res(h->mid2, tp.CAT[lm], 2 * cm);
  else plan_res(h->mid2, nullptr, cm);
  for (int u = 0; u < L - 1; ++u) {
    auto& up = h->ups[u];
    const int l = up.r1.level, co = up.r1.cout;
    plan_res(up.r1, nullptr, co); plan_res(up.r2, nullptr, co);
    plan_att(tp.att[L + 1 + u], nullptr, co);
    CvT& c = tp.ups[u];
    if (l - 1 >= 1) { c.out = tp.CAT[l - 1]; c.out_ld = 2 * h->C[l - 1]; }
    else { c.out = A.alloc<float>(B * npx(0) * h->C[0]); c.out_ld = h->C[0]; }
  }
  tp.fin_y = A.alloc<float>(B * npx(0) * h->C[0]);
  tp.fin_h = A.alloc<float>(B * npx(0) * h->C[0]);

  // ---- backward scratch ----
  tp.GA.assign(L, nullptr); tp.GB.assign(L, nullptr); tp.GY.assign(L, nullptr); tp.GY2.assign(L, nullptr); tp.GH.assign(L, nullptr);
  tp.GQKV.assign(L, nullptr); tp.GO.assign(L, nullptr); tp.GCAT.assign(L, nullptr);
  size_t wmax = 0;
  int cmax = 0;
  for (int l = 0; l < L; ++l) {
    const size_t n = npx(l);
    const size_t cw = (size_t)(l > 0 ? 2 * h->C[l] : h->C[l]);   // widest tensor at this level (concat input)
    tp.GA[l] = A.alloc<float>(B * n * cw);
    tp.GB[l] = A.alloc<float>(B * n * cw);
    tp.GY[l] = A.alloc<float>(B * n * h->C[l]);
    tp.GY2[l] = A.alloc<float>(B * n * h->C[l]);     // block1's gradient: block2's weight-gradient launch may still be reading GY (BwdCtx)
    tp.GH[l] = A.alloc<float>(B * n * h->C[l]);
    tp.GQKV[l] = A.alloc<float>(B * n * 3 * kHidden);
    tp.GO[l] = A.alloc<float>(B * n * kHidden);
    if (l > 0) tp.GCAT[l] = A.alloc<float>(B * n * 2 * h->C[l]);
    if (h->C[l] > cmax) cmax = h->C[l];
  }
  for (auto& s : h->slots)
    if (s->kind != Kind::RAW && s->buf.n > wmax) wmax = s->buf.n;
  if ((size_t)3 * kHidden * cmax > wmax) wmax = (size_t)3 * kHidden * cmax;
  tp.wscratch_floats = wmax;
  for (int k = 0; k < (h->wgrad_side_streams > 1 ? h->wgrad_side_streams : 1); ++k) {
    tp.wscratch[k] = A.alloc<float>(wmax);
    tp.M1[k] = A.alloc<float>(B * (size_t)cmax * kHidden);
    tp.colsumG[k] = A.alloc<float>((size_t)2 * cmax);
  }
  tp.weff_dg = A.alloc<float>(B * (size_t)cmax * kHidden);
  // the small accumulators a backward pass starts from zero, allocated back to back: ONE fill at its start covers all of them (they were
  // 5 fills plus one per attention block, in the middle of the data-gradient chain)
  tp.gsum = A.alloc<double>((size_t)(2 * h->n_resnets + 1) * B * kGroups * 2);
  tp.gctx_stride = B * kHeads * kDimHead * kDimHead;
  tp.gctx = A.alloc<float>(tp.gctx_stride * (tp.att.size() ? tp.att.size() : 1));     // one [B][4][32][32] block per attention
  size_t tsum = 0;
  for (size_t i = 0; i < tp.fb.tproj_off.size(); ++i) tsum = tp.fb.tproj_off[i] > tsum ? tp.fb.tproj_off[i] : tsum;
  tp.gtproj = A.alloc<float>(tsum + B * (size_t)cmax);     // same layout as fb.tproj
  tp.gtemb = A.alloc<float>(B * (h->cfg.dim + h->cfg.spk_emb_dim));
  tp.gmlp_h = A.alloc<float>(B * 4 * h->cfg.dim);
  tp.amax = A.alloc<float>(Tape::kAmaxSlots);
  tp.zero_lo = reinterpret_cast<float*>(tp.gsum);
  // the span from the POINTERS (Arena::alloc aligns before it hands out: an offset taken before the first allocation can sit below gsum)
  tp.zero_floats = (size_t)(reinterpret_cast<char*>(tp.amax + Tape::kAmaxSlots) - reinterpret_cast<char*>(tp.gsum)) / sizeof(float);
  tp.red_partials = A.alloc<double>((size_t)kRedBlocks * tp.att.size() + (size_t)final_bwd_blocks(Bp, F, T, h->C[0]) * B);
  tp.mask_copy = A.alloc<float>(B * (size_t)T);
  tp.gscaled = A.alloc<float>(B * (size_t)F * T);
}

// ---- training forward: the walk of unet_forward over the tape ---------------------------------------------------------------
inline hipError_t train_forward(us_decoder* h, Tape& tp, hipStream_t s, const float* x, const float* mu, const float* mask, const float* t,
                                const float* spk, float* out) {
  const int T = tp.T, Bp = tp.Bp;
  CK(hipMemcpyAsync(tp.mask_copy, mask, sizeof(float) * (size_t)Bp * T, hipMemcpyDeviceToDevice, s));
  tp.mask = tp.mask_copy; tp.Bm = Bp;
  EvalCtx e{h, s, &tp.fb, Bp, T, tp.mask, Bp};
  e.splitk_by_batch = 1;
  CK(zero_f64(tp.stats, tp.stats_count, s));     // every GroupNorm's partial sums of this forward
  CK(time_embedding(e, t, spk));
  CK(unet_forward(e, tp, x, Bp, mu, Bp, 0, out));
  tp.forward_done = true;
  return hipSuccess;
}

// ---- backward -------------------------------------------------------------------------------------------------
// The weight-gradient chain of a convolution (max |gy| -> zero scratch -> wgrad -> unpack into the parameter's gradient) has no consumer
// inside the backward pass, so it runs on the handle's second stream `ws` beside the data-gradient chain on `s`: at a 176-frame crop
// both are made of 5-30 us launches that leave most of the chip idle.  Ordering is by events, both ways:
//   wgrad_fork   : `ws` waits for what `s` has produced so far (gy and its amax word);
//   wgrad_done   : marks the buffer the chain read as busy until the chain's last launch;
//   acquire(buf) : called before `s` writes into a gradient buffer: waits for the chain that still reads it;
//   join         : `s` waits for everything on `ws` (always, also on the error path: a HIP graph capture must see both streams rejoin).
// ws == s (US_WGRAD_STREAM=0): the same launches in program order on one stream, no events.
struct BwdCtx {
  us_decoder* h; hipStream_t s; Tape* tp; EvalCtx* e;
  std::vector<hipStream_t> sides;          // empty: everything on `s`
  hipStream_t ws = nullptr;                // stream of the current chain (between wgrad_fork and wgrad_done)
  int cur = 0;                             // its index: selects the chain's scratch set
  unsigned used = 0;                       // side streams with work since the last join
  size_t ev_next = 0;
  std::vector<std::pair<const void*, hipEvent_t>> busy;
  bool two_streams() const { return !sides.empty(); }
  float* wscratch() const { return tp->wscratch[cur]; }
  float* M1() const { return tp->M1[cur]; }
  float* colsumG() const { return tp->colsumG[cur]; }
  hipError_t next_event(hipEvent_t* ev) {
    if (ev_next >= h->wgrad_events.size()) {
      hipEvent_t n = nullptr;
      hipError_t err = hipEventCreateWithFlags(&n, hipEventDisableTiming);
      if (err != hipSuccess) return err;
      h->wgrad_events.push_back(n);
    }
    *ev = h->wgrad_events[ev_next++];
    return hipSuccess;
  }
  hipError_t wgrad_fork() {                // chains go round-robin over the side streams
    if (!two_streams()) return hipSuccess;
    cur = (cur + 1) % (int)sides.size();
    ws = sides[(size_t)cur];
    hipEvent_t ev;
    hipError_t err = next_event(&ev);
    if (err == hipSuccess) err = hipEventRecord(ev, s);
    if (err == hipSuccess) err = hipStreamWaitEvent(ws, ev, 0);
    if (err == hipSuccess) used |= 1u << cur;
    return err;
  }
  hipError_t wgrad_done(const void* read_buf) { return wgrad_done(&read_buf, 1); }
  // one event for a chain that read several buffers
  hipError_t wgrad_done(const void* const* read_bufs, int n) {
    if (!two_streams()) return hipSuccess;
    hipEvent_t ev;
    hipError_t err = next_event(&ev);
    if (err == hipSuccess) err = hipEventRecord(ev, ws);
    if (err == hipSuccess)
      for (int i = 0; i < n; ++i)
        if (read_bufs[i]) busy.emplace_back(read_bufs[i], ev);
    return err;
  }
  // a chain the caller opens and closes itself (several parameters' launches behind ONE fork and ONE done event: the event calls are
  // ~7 us of host time each and a barrier packet each on the device); conv_wgrad then neither forks nor marks
  int manual = 0;
  hipError_t chain_begin() { hipError_t e = wgrad_fork(); ++manual; return e; }
  hipError_t chain_end(const void* const* read_bufs, int n) { --manual; return wgrad_done(read_bufs, n); }
  hipError_t acquire(const void* buf) {
    for (size_t i = 0; i < busy.size();) {
      if (busy[i].first != buf) { ++i; continue; }
      hipError_t err = hipStreamWaitEvent(s, busy[i].second, 0);
      if (err != hipSuccess) return err;
      busy.erase(busy.begin() + (long)i);
    }
    return hipSuccess;
  }
  hipError_t join() {
    hipError_t first = hipSuccess;
    busy.clear();
    for (size_t k = 0; k < sides.size(); ++k) {
      if (!(used & (1u << k))) continue;
      hipEvent_t ev;
      hipError_t err = next_event(&ev);
      if (err == hipSuccess) err = hipEventRecord(ev, sides[k]);
      if (err == hipSuccess) err = hipStreamWaitEvent(s, ev, 0);
      if (err != hipSuccess && first == hipSuccess) first = err;
    }
    used = 0;
    return first;
  }
};

// Pixels per wgrad workgroup: every workgroup ends with a 64x64 LDS reduction and 4,096 atomics, so the pixel range is
// split only as far as needed to put ~1,536 workgroups on the chip (768 at one crop): the 1,024-channel layers of a
// 176-frame crop (220 pixels, 2,304 tile-taps) take their pixels in one piece, level 0 (14,080 pixels, 36 tile-taps) in ~40.
inline int wgrad_chunk(int Ms, int cout, int cin, int ntaps, int B) {
  // one crop: 768 (the weight-gradient launches run beside the data-gradient chain on the second stream: 1,536 workgroups each took the
  // chip away from it -- fine-tune iteration 10.14 ms at 1,536, 9.78 at 768, 9.94 at 512, 10.65 at 256); a batch: 1,536 (pre-training
  // step at 32 crops: 56.0 ms at 1,536, 58.1 at 768, 60.1 at 512)
  const int target = B == 1 ? 768 : 1536;
  const long long tt = (long long)((cout + 63) / 64) * ((cin + 63) / 64) * ntaps * B;
  long long nch = (target + tt - 1) / tt;
  if (nch < 1) nch = 1;
  long long chunk = (Ms + nch - 1) / nch;
  if (chunk < 64) chunk = 64;
  chunk = (chunk + 7) / 8 * 8;
  return (int)chunk;
}

// weight + bias gradient of a forward conv with the given geometry; gy: gradient w.r.t. the conv output
// max |gy| of a gradient tensor [B][Hout][Wout][C] for the f16x3 weight-gradient kernel's scale (null on the exact-fp32 handle)
inline hipError_t wgrad_amax(BwdCtx& c, const float* gy, int gy_ld, long long rows, int C, const float** out, hipStream_t stream) {
  Tape& tp = *c.tp;
  *out = nullptr;
  if (c.h->exact) return hipSuccess;
  if (tp.amax_next >= Tape::kAmaxSlots) return hipErrorInvalidValue;
  float* slot = tp.amax + tp.amax_next++;
  *out = slot;
  return launch_wgrad_amax(gy, gy_ld, rows, C, slot, stream);
}

// amax_reuse: the maximum of the same gy taken by an earlier call (the four phase launches of a transposed convolution)
inline hipError_t conv_wgrad(BwdCtx& c, const ConvW& w, const ConvArgs& fwd, const float* gy, int gy_ld, const float* x, int x_ld,
                             bool zero_scratch, bool finish, bool oihw, int taps_total, const float** amax_reuse = nullptr) {
  Tape& tp = *c.tp;
  if (!w.w->grad) return hipSuccess;
  WgradArgs a;
  memset(&a, 0, sizeof a);
  a.exact = c.h->exact ? 1 : 0;
  // the chain of one parameter starts at the launch that may zero the scratch and ends at the one that unpacks it (the four phase
  // launches of a transposed convolution are one chain: up_backward forks before its own zero-fill)
  if (zero_scratch && !c.manual) CK(c.wgrad_fork());
  if (amax_reuse && *amax_reuse) a.gy_amax = *amax_reuse;
  else {
    CK(wgrad_amax(c, gy, gy_ld, (long long)fwd.B * fwd.Hout * fwd.Wout, w.cout, &a.gy_amax, c.ws));
    if (amax_reuse) *amax_reuse = a.gy_amax;
  }
  a.gy = gy; a.gy_ld = gy_ld; a.x = x; a.x_ld = x_ld; a.gw = c.wscratch();
  a.B = fwd.B; a.Hin = fwd.Hin; a.Win = fwd.Win; a.Cin = w.cin; a.Hout = fwd.Hout; a.Wout = fwd.Wout; a.Cout = w.cout;
  a.Hs = fwd.Hs; a.Ws = fwd.Ws; a.oy0 = fwd.oy0; a.ox0 = fwd.ox0; a.ostep = fwd.ostep; a.istride = fwd.istride; a.ntaps = fwd.ntaps;
  a.dy_bits = fwd.dy_bits; a.dx_bits = fwd.dx_bits; a.wtap_bits = fwd.wtap_bits;
  a.chunk = wgrad_chunk(fwd.Hs * fwd.Ws, w.cout, w.cin, fwd.ntaps, fwd.B);
  // a launch that covers all `taps_total` taps with one writer per element needs no zeroed scratch
  if (zero_scratch && fwd.ntaps == taps_total && launch_wgrad_single_writer(a)) a.overwrite = 1;
  else if (zero_scratch) CK(zero_f32(c.wscratch(), (size_t)taps_total * w.cout * w.cin, c.ws));
  CK(launch_wgrad(a, c.ws));
  // the convolution weights are 99.9 % of the gradient bytes: the inverse loss scale of us_estimator_backward rides in this pass (the
  // small tensors are scaled back by one table-driven launch at the end, train_abi.inc)
  if (finish) {
    CK(launch_unpack_wgrad(c.wscratch(), w.w->grad, w.cout, w.cin, taps_total, oihw, c.ws, tp.unscale));
    if (tp.unscale) w.w->grad_unscaled = true;
    if (!c.manual) CK(c.wgrad_done(gy));
  }
  return hipSuccess;
}

inline ConvArgs geom3x3(EvalCtx& e, const ConvW& w, int level) {
  const int H = e.h->cfg.n_feats >> level, W = e.T >> level;
  ConvArgs a = base_args(e, w, nullptr, 0, H, W, nullptr, 0, H, W);
  a.ntaps = 9;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) a.set_tap(ky * 3 + kx, ky - 1, kx - 1, ky * 3 + kx);
  return a;
}
inline ConvArgs geom1x1(EvalCtx& e, const ConvW& w, int level) {
  const int H = e.h->cfg.n_feats >> level, W = e.T >> level;
  ConvArgs a = base_args(e, w, nullptr, 0, H, W, nullptr, 0, H, W);
  a.ntaps = 1;
  a.set_tap(0, 0, 0, 0);
  return a;
}

// data gradient of a stride-1 conv (3x3 or 1x1): gx = conv(gy, W^T flipped) [+ add] [* mask]
inline hipError_t conv_dgrad_s1(BwdCtx& c, const Slot* wslot, int cin, int cout, int k, const float* gy, int gy_ld, int level, float* gx,
                                int gx_ld, const float* add, int add_ld, const float* alpha, bool mask_out, const float* wt_override,
                                long long wt_bstride, int bk_override) {
  EvalCtx& e = *c.e;
  const int H = e.h->cfg.n_feats >> level, W = e.T >> level;
  CK(c.acquire(gx));
  if (k == 3 && !wt_override && !alpha && wslot->wino_dg.p && e.b->wino_v) {
    // the data gradient of a Winograd-domain conv is one too: conv of gy with the rotated, channel-swapped filter
    WinoEpi ep;
    ep.add = add; ep.add_ld = add_ld; ep.mask_out = mask_out;
    return wino_conv(e, gy, gy_ld, wslot->wino_dg.p, cout, cin, wslot->bk_dg, level, gx, gx_ld, ep, nullptr, wslot->wino_dg_f16);
  }
  ConvArgs a;
  memset(&a, 0, sizeof a);
  a.in = gy; a.in_ld = gy_ld; a.out = gx; a.out_ld = gx_ld;
  a.wt = wt_override ? wt_override : wslot->dg.p;
  a.wt_bstride = wt_bstride;
  a.bk = wt_override ? bk_override : wslot->bk_dg;
  a.f16 = (!wt_override && wslot->dg_f16) ? 2 : 0;      // f16x3, the fp32 gradient split inside the kernel
  a.B = e.Bp; a.Hin = H; a.Win = W; a.Cin = cout; a.Hout = H; a.Wout = W; a.Cout = cin;
  a.Hs = H; a.Ws = W; a.ostep = 1; a.istride = 1;
  a.omask_bmod = 1; a.zeros = e.h->zeros;
  a.splitk_ws = e.b->splitk; a.splitk_ws_floats = (long long)e.b->splitk_floats; a.splitk_by_batch = 1;
  a.ntaps = k * k;
  for (int ky = 0; ky < k; ++ky)
    for (int kx = 0; kx < k; ++kx) a.set_tap(ky * k + kx, k == 3 ? 1 - ky : 0, k == 3 ? 1 - kx : 0, ky * k + kx);
  a.add = add; a.add_ld = add_ld; a.alpha = alpha;
  if (mask_out) set_omask(e, a, level);
  return run_conv(e, a);
}

// amax_out (optional): receives a word holding max |gy|, taken inside the second pass: the weight-gradient launch that consumes gy
// needs no pass of its own (conv_wgrad's amax_reuse)
inline hipError_t gn_backward(BwdCtx& c, const float* y, int C, int level, const double* stats, const Slot* gamma, const Slot* beta,
                              const float* g, int g_ld, float* gy, const Slot* conv_bias, const float** amax_out = nullptr) {
  EvalCtx& e = *c.e;
  Tape& tp = *c.tp;
  if (!gamma->grad || !beta->grad) return hipErrorInvalidValue;
  CK(c.acquire(gy));
  double* gsum = tp.gsum + (size_t)(tp.gsum_next++) * e.Bp * kGroups * 2;      // zeroed at the start of the backward pass
  GnBwdArgs a;
  memset(&a, 0, sizeof a);
  a.y = y; a.y_ld = C; a.stats = stats; a.gamma = gamma->buf.p; a.beta = beta->buf.p;
  a.g = g; a.g_ld = g_ld;
  a.mask = e.mask; a.mask_ld = e.T; a.mask_step = 1 << level; a.mask_bmod = e.Bm;
  a.gy = gy; a.gy_ld = C;
  a.ggamma = gamma->grad; a.gbeta = beta->grad;
  a.gbias = conv_bias ? conv_bias->grad : nullptr;
  a.gsum = gsum;
  a.B = e.Bp; a.H = e.h->cfg.n_feats >> level; a.W = e.T >> level; a.C = C;
  if (amax_out) {
    *amax_out = nullptr;
    if (!c.h->exact && tp.amax_next < Tape::kAmaxSlots) {
      a.gy_amax = tp.amax + tp.amax_next++;
      *amax_out = a.gy_amax;
    }
  }
  return launch_gn_bwd(a, c.s);
}

// bias gradient of a convolution (column sums of the gradient w.r.t. its output): nothing in the backward pass reads it -> second stream
inline hipError_t side_colsum(BwdCtx& c, const float* G, int g_ld, long long rows, int C, float* out) {
  if (c.manual) return launch_colsum(G, g_ld, rows, C, nullptr, out, c.ws);
  CK(c.wgrad_fork());
  CK(launch_colsum(G, g_ld, rows, C, nullptr, out, c.ws));
  return c.wgrad_done(G);
}

// ResnetBlock backward.  G: gradient w.r.t. the stored output (ld g_ld).  gx: gradient w.r.t. the stored input
// (always a pre-masked tensor -> masked); null for the first (2-channel) block.
inline hipError_t resnet_backward(BwdCtx& c, const ResT& t, const float* G, int g_ld, float* gx, int gx_ld) {
  EvalCtx& e = *c.e;
  Tape& tp = *c.tp;
  const ResnetW& r = *t.w;
  const int l = r.level, co = r.cout;
  const long long n = (long long)(e.h->cfg.n_feats >> l) * (e.T >> l);
  float* GY = tp.GY[l];
  float* GH = tp.GH[l];
  // block2
  const float* amax_gy = nullptr;
  CK(gn_backward(c, t.y2, co, l, t.st2, r.g2, r.b2, G, g_ld, GY, r.c2.b, &amax_gy));
  ConvArgs g2 = geom3x3(e, r.c2, l);
  CK(conv_wgrad(c, r.c2, g2, GY, co, t.h1, co, true, true, true, 9, &amax_gy));
  CK(conv_dgrad_s1(c, r.c2.w, r.c2.cin, r.c2.cout, 3, GY, co, l, GH, co, nullptr, 0, nullptr, true, nullptr, 0, 0));
  GY = tp.GY2[l];            // block1's gradient in its own buffer: block2's weight-gradient chain may still be reading the first
  // time-embedding projection: h1 = (a1*m + tproj)*m  ->  gtproj[b][c] = sum_p GH (already masked)
  // (no consumer before the MLP backward at the very end: on the second stream, GH marked busy until it has been read)
  // (one crop only: the event calls weigh where launches are 5-30 us -- fine-tune iteration 9.32 -> 9.26 ms; at 32 crops starting the row
  // sums and block1's weight gradient later costs overlap: pre-training step 55.4 -> 56.2 ms)
  const bool merged = !r.first && e.Bp == 1;      // the row sums wait for block1's chain below (GH stays untouched until the next block)
  if (!merged) {
    CK(c.wgrad_fork());
    CK(launch_rowsum_per_item(GH, co, e.Bp, n, co, tp.gtproj + tp.fb.tproj_off[r.index], c.ws));
    CK(c.wgrad_done(GH));
  }
  // block1
  amax_gy = nullptr;
  CK(gn_backward(c, t.y1, co, l, t.st1, r.g1, r.b1, GH, co, GY, r.c1.b, &amax_gy));
  if (r.first) {
    CK(launch_first_conv_wgrad(tp.fb.in2, GY, G, e.Bp, e.h->cfg.n_feats, e.T, co, r.c1.w->grad, r.res.w->grad, c.s));
    CK(launch_colsum(G, g_ld, (long long)e.Bp * n, co, nullptr, r.res.b->grad, c.s));
    // d loss / d x and d loss / d mu (callers that train an encoder through the decoder, train_STEP1.py:381, train_STEP2.py:299)
    if ((tp.grad_x || tp.grad_mu) && g_ld == co)
      CK(launch_first_conv_dgrad(GY, G, r.c1.w->buf.p, r.res.w->buf.p, tp.mask, tp.grad_mu, tp.grad_x, e.Bp, e.h->cfg.n_feats, e.T, co, c.s));
    else if (tp.grad_x || tp.grad_mu)
      return hipErrorInvalidValue;
    return hipSuccess;
  }
  ConvArgs g1 = geom3x3(e, r.c1, l);
  // everything else of the block that only feeds parameter gradients, behind one fork and one event: the time-projection row sums
  // (GH), block1's weight gradient (GY), res_conv's weight and bias gradients (G)
  if (merged) {
    CK(c.chain_begin());
    CK(launch_rowsum_per_item(GH, co, e.Bp, n, co, tp.gtproj + tp.fb.tproj_off[r.index], c.ws));
  }
  CK(conv_wgrad(c, r.c1, g1, GY, co, t.x, t.x_ld, true, true, true, 9, &amax_gy));
  if (r.has_res) {
    ConvArgs gr = geom1x1(e, r.res, l);
    CK(conv_wgrad(c, r.res, gr, G, g_ld, t.x, t.x_ld, true, true, true, 1));
    CK(side_colsum(c, G, g_ld, (long long)e.Bp * n, co, r.res.b->grad));
  }
  if (merged) {
    const void* bufs[3] = {GH, GY, r.has_res ? G : nullptr};
    CK(c.chain_end(bufs, 3));
  }
  if (r.has_res) {
    CK(conv_dgrad_s1(c, r.res.w, r.res.cin, r.res.cout, 1, G, g_ld, l, gx, gx_ld, nullptr, 0, nullptr, false, nullptr, 0, 0));
    CK(conv_dgrad_s1(c, r.c1.w, r.c1.cin, r.c1.cout, 3, GY, co, l, gx, gx_ld, gx, gx_ld, nullptr, true, nullptr, 0, 0));
  } else {
    CK(conv_dgrad_s1(c, r.c1.w, r.c1.cin, r.c1.cout, 3, GY, co, l, gx, gx_ld, G, g_ld, nullptr, true, nullptr, 0, 0));
  }
  return hipSuccess;
}

// Residual(Rezero(LinearAttention)) backward.  G: gradient w.r.t. the stored (masked) output; gx: gradient w.r.t. the
// raw input (unmasked).  Algebra (per item, O = ctx^T q folded as W_eff q, ctx = softmax_n(k)^T v):
//   out = (x + g*(W_eff q + b_o)) * m
//   M1 = G^T q;  g_Wo = g * M1 ctx;  g_bo = g * colsum(G);  g_g = sum(G * (W_eff q + b_o)) as autograd forms it: a fixed-order fp64 sum over the
//   stored fn(x) (AttT::o_pre), finished by launch_reduce_finalize at the end of the pass (train.hip)
//   gO = g * G W_o;  g_q = g * G W_eff;  g_ctx = q^T gO;  (g_k, g_v) from softmax/ctx backward;  g_x = G + g_qkv W_qkv
inline hipError_t attention_backward(BwdCtx& c, const AttT& t, const float* G, int g_ld, float* gx, int gx_ld) {
  EvalCtx& e = *c.e;
  Tape& tp = *c.tp;
  const AttnW& at = *t.w;
  const int l = at.level, C = at.dim;
  const int H = e.h->cfg.n_feats >> l, W = e.T >> l;
  const int n = H * W;
  const float* gptr = at.g->buf.p;
  // bias / Rezero gain / to_out weight: parameter gradients only (colsumG and M1 are scratch of this chain) -> second stream
  CK(c.wgrad_fork());
  hipStream_t as = c.ws;
  CK(zero_f32(c.colsumG(), (size_t)C, as));
  CK(launch_colsum(G, g_ld, (long long)e.Bp * n, C, nullptr, c.colsumG(), as));
  CK(launch_attn_bwd_bias(c.colsumG(), at.out_b->buf.p, gptr, C, at.out_b->grad, nullptr, as));
  CK(launch_dot_partial(G, g_ld, t.o_pre, C, (long long)e.Bp * n, C, tp.red_partials + (size_t)(&t - tp.att.data()) * kRedBlocks, as));
  // M1[b] = G^T q  (per item)
  CK(zero_f32(c.M1(), (size_t)e.Bp * C * kHidden, as));
  {
    WgradArgs a;
    memset(&a, 0, sizeof a);
    a.exact = c.h->exact ? 1 : 0;
    CK(wgrad_amax(c, G, g_ld, (long long)e.Bp * n, C, &a.gy_amax, as));
    a.gy = G; a.gy_ld = g_ld; a.x = t.qkv; a.x_ld = 3 * kHidden; a.gw = c.M1(); a.gw_bstride = (long long)C * kHidden;
    a.B = e.Bp; a.Hin = H; a.Win = W; a.Cin = kHidden; a.Hout = H; a.Wout = W; a.Cout = C;
    a.Hs = H; a.Ws = W; a.ostep = 1; a.istride = 1; a.ntaps = 1;
    a.set_tap(0, 0, 0, 0);
    a.chunk = wgrad_chunk(n, C, kHidden, 1, e.Bp);
    CK(launch_wgrad(a, as));
  }
  CK(launch_attn_bwd_wout(c.M1(), t.ctx, at.out_w->buf.p, gptr, e.Bp, C, at.out_w->grad, nullptr, as));
  CK(c.wgrad_done(G));
  // gO = g * G W_o   [n x 128]
  float* gO = tp.GO[l];
  CK(conv_dgrad_s1(c, at.out_w, kHidden, C, 1, G, g_ld, l, gO, kHidden, nullptr, 0, gptr, false, nullptr, 0, 0));
  // g_ctx, then (g_k, g_v)
  float* gqkv = tp.GQKV[l];
  CK(c.acquire(gqkv));
  float* gctx = tp.gctx + (size_t)(&t - tp.att.data()) * tp.gctx_stride;       // this block's own accumulator, zero since the pass began
  CK(launch_attn_bwd_gctx(t.qkv, gO, e.Bp, n, gctx, c.s));
  CK(launch_attn_bwd_kv(t.qkv, t.ctx, gctx, t.colM, t.colS, e.Bp, n, gqkv, c.s));
  // g_q = g * G W_eff (per-item weights)
  const int bkc = pick_bk(C);
  CK(launch_attn_weff_dgrad(t.ctx, at.out_w->buf.p, tp.weff_dg, e.Bp, C, bkc, c.s));
  CK(conv_dgrad_s1(c, nullptr, kHidden, C, 1, G, g_ld, l, gqkv, 3 * kHidden, nullptr, 0, gptr, false, tp.weff_dg, (long long)C * kHidden, bkc));
  // to_qkv: weight gradient and data gradient (+ residual)
  ConvArgs gq = geom1x1(e, at.qkv, l);
  CK(conv_wgrad(c, at.qkv, gq, gqkv, 3 * kHidden, t.x, t.x_ld, true, true, true, 1));
  CK(conv_dgrad_s1(c, at.qkv.w, at.qkv.cin, at.qkv.cout, 1, gqkv, 3 * kHidden, l, gx, gx_ld, G, g_ld, nullptr, false, nullptr, 0, 0));
  return hipSuccess;
}

// Downsample (Conv2d 3x3 stride 2, level l -> l+1) backward.  G: gradient w.r.t. the (masked) output at level l+1.
// gx (level l) = [add +] conv_transpose(G), masked.
inline hipError_t down_backward(BwdCtx& c, const CvT& t, const float* G, int g_ld, float* gx, int gx_ld, const float* add, int add_ld) {
  EvalCtx& e = *c.e;
  const ConvW& w = *t.w;
  const int l = t.level;
  const int H = e.h->cfg.n_feats >> l, W = e.T >> l;
  const long long n_out = (long long)(H / 2) * (W / 2);
  // weight / bias gradient with the forward geometry
  ConvArgs f = base_args(e, w, nullptr, 0, H, W, nullptr, 0, H / 2, W / 2);
  f.ntaps = 9; f.istride = 2;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) f.set_tap(ky * 3 + kx, ky - 1, kx - 1, ky * 3 + kx);
  const bool one_chain = e.Bp == 1;          // weight and bias gradient behind one fork / one event (one crop, as in resnet_backward)
  if (one_chain) CK(c.chain_begin());
  CK(conv_wgrad(c, w, f, G, g_ld, t.x, t.x_ld, true, true, true, 9));
  CK(side_colsum(c, G, g_ld, (long long)e.Bp * n_out, w.cout, w.b->grad));
  if (one_chain) {
    const void* bufs[1] = {G};
    CK(c.chain_end(bufs, 1));
  }
  CK(c.acquire(gx));
  // data gradient: input row iy = 2*oy - 1 + ky.  Phase py = iy & 1: py=0 -> (ky=1, oy=m); py=1 -> (ky=0, oy=m+1), (ky=2, oy=m)
  static const int NT[2] = {1, 2};
  static const int KY[2][2] = {{1, 0}, {0, 2}};
  static const int DY[2][2] = {{0, 0}, {1, 0}};
  for (int py = 0; py < 2; ++py)
    for (int px = 0; px < 2; ++px) {
      ConvArgs a;
      memset(&a, 0, sizeof a);
      a.in = G; a.in_ld = g_ld; a.out = gx; a.out_ld = gx_ld;
      a.wt = w.w->dg.p; a.bk = w.w->bk_dg; a.f16 = w.w->dg_f16 ? 2 : 0;
      a.B = e.Bp; a.Hin = H / 2; a.Win = W / 2; a.Cin = w.cout; a.Hout = H; a.Wout = W; a.Cout = w.cin;
      a.Hs = H / 2; a.Ws = W / 2; a.ostep = 2; a.oy0 = py; a.ox0 = px; a.istride = 1;
      a.omask_bmod = 1; a.zeros = e.h->zeros;
      a.splitk_ws = e.b->splitk; a.splitk_ws_floats = (long long)e.b->splitk_floats; a.splitk_by_batch = 1;
      int nt = 0;
      for (int i = 0; i < NT[py]; ++i)
        for (int j = 0; j < NT[px]; ++j) a.set_tap(nt++, DY[py][i], DY[px][j], KY[py][i] * 3 + KY[px][j]);
      a.ntaps = nt;
      a.add = add; a.add_ld = add_ld;
      set_omask(e, a, l);
      CK(run_conv(e, a));
    }
  return hipSuccess;
}

// Upsample (ConvTranspose2d 4x4 stride 2, level l -> l-1) backward.  G: gradient w.r.t. the (masked) output at level l-1.
inline hipError_t up_backward(BwdCtx& c, const CvT& t, const float* G, int g_ld, float* gx, int gx_ld) {
  EvalCtx& e = *c.e;
  Tape& tp = *c.tp;
  const ConvW& w = *t.w;
  const int l = t.level;
  const int H = e.h->cfg.n_feats >> l, W = e.T >> l;
  static const int KY[2][2] = {{1, 3}, {2, 0}};
  static const int DY[2][2] = {{0, -1}, {0, 1}};
  if (w.w->grad) {
    CK(c.wgrad_fork());
    CK(zero_f32(c.wscratch(), (size_t)16 * w.cout * w.cin, c.ws));
    const float* amax_g = nullptr;
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        ConvArgs f = base_args(e, w, nullptr, 0, H, W, nullptr, 0, 2 * H, 2 * W);
        f.Hs = H; f.Ws = W; f.ostep = 2; f.oy0 = py; f.ox0 = px; f.ntaps = 4;
        for (int i = 0; i < 2; ++i)
          for (int j = 0; j < 2; ++j) f.set_tap(i * 2 + j, DY[py][i], DY[px][j], KY[py][i] * 4 + KY[px][j]);
        CK(conv_wgrad(c, w, f, G, g_ld, t.x, t.x_ld, false, py == 1 && px == 1, false, 16, &amax_g));
      }
  }
  CK(side_colsum(c, G, g_ld, (long long)e.Bp * (2 * H) * (2 * W), w.cout, w.b->grad));
  CK(c.acquire(gx));
  // data gradient: gx[iy][ix][ci] = sum_{ky,kx,co} G[2*iy-1+ky][2*ix-1+kx][co] * W[ci][co][ky][kx]
  ConvArgs a;
  memset(&a, 0, sizeof a);
  a.in = G; a.in_ld = g_ld; a.out = gx; a.out_ld = gx_ld;
  a.wt = w.w->dg.p; a.bk = w.w->bk_dg; a.f16 = w.w->dg_f16 ? 2 : 0;
  a.B = e.Bp; a.Hin = 2 * H; a.Win = 2 * W; a.Cin = w.cout; a.Hout = H; a.Wout = W; a.Cout = w.cin;
  a.Hs = H; a.Ws = W; a.ostep = 1; a.istride = 2;
  a.omask_bmod = 1; a.zeros = e.h->zeros;
  a.splitk_ws = e.b->splitk; a.splitk_ws_floats = (long long)e.b->splitk_floats; a.splitk_by_batch = 1;
  a.ntaps = 16;
  for (int ky = 0; ky < 4; ++ky)
    for (int kx = 0; kx < 4; ++kx) a.set_tap(ky * 4 + kx, ky - 1, kx - 1, ky * 4 + kx);
  set_omask(e, a, l);
  return run_conv(e, a);
}

inline hipError_t train_backward_body(us_decoder* h, Tape& tp, BwdCtx& c, EvalCtx& e, const float* grad_out, bool grads_zeroed) {
  const int L = h->cfg.n_mults, F = h->cfg.n_feats, T = tp.T, Bp = tp.Bp;
  hipStream_t s = c.s;
  const int c0 = h->C[0];
  auto npx = [&](int l) { return (long long)(F >> l) * (T >> l); };
  tp.gsum_next = 0;
  tp.amax_next = 0;
  CK(zero_f32(tp.zero_lo, tp.zero_floats, s));          // every small accumulator of the pass (plan_train)
  // zero every requested parameter gradient and the time-projection gradient block
  if (!grads_zeroed)
    for (auto& sl : h->slots)
      if (sl->grad) CK(zero_f32(sl->grad, sl->buf.n, s));
  // ---- final block (unitspeech.py:198-201) ----
  float* GH0 = tp.GH[0];
  double* fin_partials = tp.red_partials + (size_t)kRedBlocks * tp.att.size();
  CK(launch_final_bwd(grad_out, tp.fin_h, c0, h->final_w1->buf.p, tp.mask, T, tp.Bm, GH0, h->final_w1->grad, fin_partials, Bp, F, T, c0, s));
  float* GY0 = tp.GY[0];
  const float* amax_fin = nullptr;
  CK(gn_backward(c, tp.fin_y, c0, 0, tp.fin_st, h->final_g, h->final_b, GH0, c0, GY0, h->final_conv3.b, &amax_fin));
  ConvArgs gf = geom3x3(e, h->final_conv3, 0);
  CK(conv_wgrad(c, h->final_conv3, gf, GY0, c0, tp.fin_x, tp.fin_ld, true, true, true, 9, &amax_fin));
  // gradient w.r.t. the last Upsample output (or mid2 output when there are no ups)
  float* gfin = tp.GA[0];
  int gfin_ld = c0;
  if (L == 1) { gfin = tp.GA[0]; }
  CK(conv_dgrad_s1(c, h->final_conv3.w, c0, c0, 3, GY0, c0, 0, gfin, gfin_ld, nullptr, 0, nullptr, true, nullptr, 0, 0));

  // ---- ups, shallow to deep ----
  const float* g_up_out = gfin;     // gradient w.r.t. ups[u]'s Upsample output
  int g_up_ld = gfin_ld;
  size_t ai = tp.att.size();
  for (int u = L - 2; u >= 0; --u) {
    auto& up = h->ups[u];
    const int l = up.r1.level, co = up.r1.cout;
    float* gA = tp.GA[l];                       // wrt attention output [n_l x co]
    CK(up_backward(c, tp.ups[u], g_up_out, g_up_ld, gA, co));
    float* gQ = tp.GB[l];                       // wrt r2 output (raw)
    const AttT& at = tp.att[--ai];
    CK(attention_backward(c, at, gA, co, gQ, co));
    float* gP = tp.GA[l];                       // wrt r1 output (masked)
    CK(resnet_backward(c, tp.res[up.r2.index], gQ, co, gP, co));
    CK(resnet_backward(c, tp.res[up.r1.index], gP, co, tp.GCAT[l], 2 * h->C[l]));
    g_up_out = tp.GCAT[l];                      // first half: x part produced by the deeper stage
    g_up_ld = 2 * h->C[l];
  }
  // ---- mid ----
  const int lm = L - 1, cm = h->C[lm];
  float* gmid_in = tp.GA[lm];                   // wrt hidden of the last level coming through the mid blocks
  {
    const float* G2 = g_up_out;                 // wrt mid2 output (first half of GCAT[lm], or gfin when L == 1)
    int G2_ld = g_up_ld;
    float* gAtt = tp.GB[lm];
    CK(resnet_backward(c, tp.res[h->mid2.index], G2, G2_ld, gAtt, cm));
    const AttT& at = tp.att[--ai];
    float* gM1 = tp.GA[lm];
    CK(attention_backward(c, at, gAtt, cm, gM1, cm));
    float* gHid = tp.GB[lm];
    CK(resnet_backward(c, tp.res[h->mid1.index], gM1, cm, gHid, cm));
    gmid_in = gHid;
  }
  // ---- downs, deep to shallow ----
  const float* g_hid = gmid_in;                 // gradient w.r.t. the level's attention output arriving from below
  int g_hid_ld = cm;
  size_t di = tp.downs.size();
  for (int l = L - 1; l >= 0; --l) {
    auto& d = h->downs[l];
    const int cl = h->C[l];
    const float* Gat;
    int Gat_ld;
    if (l == L - 1) {
      // total = mid path + skip path (second half of GCAT[l])
      if (L > 1) {
        float* sum = tp.GA[l];
        // sum = g_hid + GCAT[l][:, cl:]  via the 1x1 path-free elementwise helper: reuse copy_rows + colwise add through conv add is
        // overkill; a strided add kernel does it
        CK(c.acquire(sum));
        CK(launch_add2(g_hid, g_hid_ld, tp.GCAT[l] + cl, 2 * cl, sum, cl, (long long)Bp * npx(l), cl, s));
        Gat = sum; Gat_ld = cl;
      } else { Gat = g_hid; Gat_ld = g_hid_ld; }
    } else {
      Gat = g_hid; Gat_ld = g_hid_ld;          // down_backward already added the skip half
    }
    const AttT& at = tp.att[--ai];
    float* gQ = tp.GB[l];
    CK(attention_backward(c, at, Gat, Gat_ld, gQ, cl));
    float* gP = tp.GA[l];
    CK(resnet_backward(c, tp.res[d.r2.index], gQ, cl, gP, cl));
    if (l == 0) {
      CK(resnet_backward(c, tp.res[d.r1.index], gP, cl, nullptr, 0));
      break;
    }
    float* gD = tp.GB[l];                       // wrt the Downsample output of level l-1  [n_l x C_{l-1}]
    CK(resnet_backward(c, tp.res[d.r1.index], gP, cl, gD, h->C[l - 1]));
    // through the Downsample of level l-1, adding the skip-connection half of that level
    const CvT& cv = tp.downs[--di];
    float* gh = tp.GA[l - 1];
    const float* add = (l - 1 >= 1) ? tp.GCAT[l - 1] + h->C[l - 1] : nullptr;
    CK(down_backward(c, cv, gD, h->C[l - 1], gh, h->C[l - 1], add, 2 * h->C[l - 1]));
    g_hid = gh; g_hid_ld = h->C[l - 1];
  }
  // ---- time / speaker embedding MLPs (unitspeech.py:165-168, 61, 72) ----
  const int dim = h->cfg.dim, S = h->cfg.spk_emb_dim, td = dim + S;
  CK(c.join());            // gtproj (the per-item row sums of every ResnetBlock) was accumulated on the second stream
  {
    // the scalar gradients: the eight Rezero gains (partials written by launch_dot_partial on the second stream) and the final bias
    RedJobs jobs;
    memset(&jobs, 0, sizeof jobs);
    for (size_t i = 0; i < tp.att.size() && jobs.count < RedJobs::kMax - 1; ++i) {
      const AttT& t = tp.att[i];
      if (!t.w->g->grad) continue;
      const long long n = npx(t.w->level);
      jobs.p[jobs.count] = tp.red_partials + i * kRedBlocks;
      jobs.n[jobs.count] = dot_partial_blocks((long long)Bp * n, t.w->dim);
      jobs.dst[jobs.count] = t.w->g->grad;
      ++jobs.count;
    }
    if (h->final_b1->grad) {
      jobs.p[jobs.count] = fin_partials;
      jobs.n[jobs.count] = final_bwd_blocks(Bp, F, T, c0) * Bp;
      jobs.dst[jobs.count] = h->final_b1->grad;
      ++jobs.count;
    }
    CK(launch_reduce_finalize(jobs, s));
  }
  auto proj_bwd = [&](const ResnetW& r) {
    return launch_linear_bwd(tp.gtproj + tp.fb.tproj_off[r.index], r.cout, r.mlp_w->buf.p, tp.fb.temb, td, Bp, td, r.cout, true,
                             r.mlp_w->grad, r.mlp_b->grad, tp.gtemb, td, s);
  };
  {
    // all 22 projections in two launches (weight / bias gradients, input gradient) instead of 44 at the tail of the pass, after the join
    std::vector<LinJob> jobs;
    std::vector<const ResnetW*> blocks;
    const int total = proj_jobs(h, jobs, blocks);
    if (h->lin_tab_bwd_dev && jobs.size() <= us_decoder::kLinJobs) {
      for (size_t i = 0; i < jobs.size(); ++i) {
        const ResnetW* r = blocks[i];
        jobs[i].gy = tp.gtproj + tp.fb.tproj_off[r->index];
        jobs[i].gW = r->mlp_w->grad; jobs[i].gb = r->mlp_b->grad;
      }
      if (upload_bytes(h, jobs.data(), jobs.size() * sizeof(LinJob), h->lin_tab_bwd_dev, s) != US_OK) return hipErrorUnknown;
      CK(launch_linear_bwd_multi(h->lin_tab_bwd_dev, (int)jobs.size(), total, tp.fb.temb, td, Bp, td, true, tp.gtemb, td, s));
    } else {
      CK(for_each_resnet(h, proj_bwd));
    }
  }
  CK(launch_mul_mish_grad(tp.gtemb, td, tp.fb.temb, td, Bp, td, s));       // mish'(temb), shared by the 22 projections
  if (tp.grad_spk) CK(launch_copy_rows(tp.gtemb + dim, td, Bp, tp.grad_spk, S, Bp, S, s));    // temb = cat(time mlp, spk_emb) (:168)
  CK(launch_linear_bwd(tp.gtemb, td, h->mlp2_w->buf.p, tp.fb.mlp_h, 4 * dim, Bp, 4 * dim, dim, true, h->mlp2_w->grad, h->mlp2_b->grad,
                       tp.gmlp_h, 4 * dim, s));
  CK(launch_mul_mish_grad(tp.gmlp_h, 4 * dim, tp.fb.mlp_h, 4 * dim, Bp, 4 * dim, s));
  CK(launch_linear_bwd(tp.gmlp_h, 4 * dim, h->mlp0_w->buf.p, tp.fb.posemb, dim, Bp, dim, 4 * dim, false, h->mlp0_w->grad, h->mlp0_b->grad,
                       nullptr, 0, s));
  return hipSuccess;
}

inline hipError_t train_backward(us_decoder* h, Tape& tp, hipStream_t s, const float* grad_out, bool grads_zeroed) {
  EvalCtx e{h, s, &tp.fb, tp.Bp, tp.T, tp.mask, tp.Bm};
  e.splitk_by_batch = 1;
  BwdCtx c{h, s, &tp, &e};
  c.ws = s;
  // Not under stream capture: a replayed HIP graph with parallel branches loses the runtime's single-queue fast path (measured: 24.9 ms
  // per fine-tune iteration against 11.1 ms for the same launches captured as one chain; DESIGN.md 7), so a capturing caller gets the chain.
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
  if (h->wgrad_side_streams > 0 && cap == hipStreamCaptureStatusNone) {
    // lowest priority: the data-gradient chain on the caller's stream is the critical path, the parameter gradients have slack until the join
    while ((int)h->wgrad_streams.size() < h->wgrad_side_streams) {
      int least = 0, greatest = 0;
      (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
      hipStream_t ns = nullptr;
      if (hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, least) != hipSuccess) { (void)hipGetLastError(); break; }
      h->wgrad_streams.push_back(ns);
    }
    c.sides = h->wgrad_streams;
  }
  hipError_t err = train_backward_body(h, tp, c, e, grad_out, grads_zeroed);
  hipError_t jerr = c.join();           // also after a failed launch: the second stream must rejoin (graph capture), and nothing may outlive the call
  return err != hipSuccess ? err : jerr;
}
