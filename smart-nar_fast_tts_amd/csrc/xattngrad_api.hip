// C-ABI of the cross-attention training forward and backward (include/nar_fs2.h ns_xg_*; transformer/SubLayers.py:8-59 used as
// FFTBlock2.crs_attn, transformer/Layers.py:61-64).  No handle: the weights are the caller's live tensors in checkpoint layout, the
// workspace, the saved activations and the attention map belong to the caller.  Host-side only; every argument is validated before the
// first HIP call.  The forward's attention is k_cross_attention as the aligner runs it; the four Linears run on what predgrad.hip and
// gemm_conv.hip already have (the column sums included), the row kernels are attngrad.hip's; the checks, the parameter table, the size
// queries, the counted GEMM launch and the column-partial finish are train_api.h's.  The launch counts are stated in the header.
#include "../../include/nar_fs2.h"
#include "train_api.h"

using namespace ns;

static_assert(sizeof(ns_xg_shape) == 20, "ns_xg_shape layout");
static_assert(sizeof(ns_xg_weights) == 10 * sizeof(void*) && sizeof(ns_xg_grads) == 12 * sizeof(void*), "ns_xg_weights / ns_xg_grads layout");

namespace {
thread_local int t_launches = 0;
thread_local const Counted counted{"ns_xg", &t_launches};

struct Ws {  // the workspace of one shape, carved in this order
  float *wkv, *bkv, *wkvt, *wqt, *wfct;  // [2d][d] and [2d] (forward), [d][2d], [d][d], [d][d] (data gradients)
  float* partial;                        // the weight gradient's per-range tiles
  double *colq, *colkv;                  // [2][row blocks of B*T][PG_SLOTS][d], [row blocks of B*L][PG_SLOTS][d]
  float *a, *b, *c;                      // [B*T, d] each: u (forward); dz, du, dctx (backward)
  float *tq, *tkv;                       // [B*T, d], [B*L, 2d]: dq, dkv (backward), q, kv of a forward that saves nothing
  float* stat;                           // [B, H, T]: D (backward)
  float* kvpart;                         // [ns_xg_kv_splits][B*L][2d], absent when there is one part
};

int check_dims(int B, int T, int L, int d, int H, const std::string& w) {
  if (B <= 0 || T <= 0 || L <= 0)
    return api_fail(w + "B, T and L must be positive, got " + std::to_string(B) + " x " + std::to_string(T) + " x " + std::to_string(L));
  if (d != 256 && d != 512) return api_fail(w + "d must be 256 or 512, got " + std::to_string(d));
  if (H <= 0 || d % H != 0) return api_fail(w + "d must be a multiple of H, got d = " + std::to_string(d) + ", H = " + std::to_string(H));
  const int dk = d / H;
  if (!cross_attention_ok(H, dk)) return api_fail(w + "d / H must be 64 or 128, got " + std::to_string(dk));
  if ((long long)B * H * T * L >= (1ll << 31)) return api_fail(w + "problem too large: B * H * T * L must stay below 2^31");
  if ((long long)B * std::max(T, L) * 2 * d >= (1ll << 31)) return api_fail(w + "problem too large: B * max(T, L) * 2d must stay below 2^31");
  return 0;
}

int carve(const ns_xg_shape& s, void* base, Ws* ws, size_t* bytes, const std::string& w) {
  const int MT = s.B * s.T, ML = s.B * s.L, d = s.d;
  PgWgradPlan pt, pl;
  if (!pg_plan_wgrad(MT, d, d, 1, &pt) || !pg_plan_wgrad(ML, d, d, 1, &pl)) return api_fail(w + "problem too large for the weight gradient's split");
  const int nsplit = xg_kv_splits(s.B, s.H, s.T, s.L);
  Bump bump(base);
  const size_t dd = (size_t)d * d, mt = (size_t)MT * d, ml = (size_t)ML * 2 * d;
  ws->wkv = bump.f(2 * dd); ws->bkv = bump.f(2 * (size_t)d); ws->wkvt = bump.f(2 * dd); ws->wqt = bump.f(dd); ws->wfct = bump.f(dd);
  ws->partial = bump.f((size_t)std::max(pt.ws_floats, pl.ws_floats));
  ws->colq = (double*)bump.raw((size_t)2 * pg_row_blocks(MT) * PG_SLOTS * d * sizeof(double));
  ws->colkv = (double*)bump.raw((size_t)pg_row_blocks(ML) * PG_SLOTS * d * sizeof(double));
  ws->a = bump.f(mt); ws->b = bump.f(mt); ws->c = bump.f(mt);
  ws->tq = bump.f(mt); ws->tkv = bump.f(ml);
  ws->stat = bump.f((size_t)s.B * s.H * s.T);
  ws->kvpart = nsplit > 1 ? bump.f((size_t)nsplit * ml) : nullptr;
  *bytes = bump.off;
  return 0;
}

int check_shape(const ns_xg_shape& s, const std::string& w) { return check_dims(s.B, s.T, s.L, s.d, s.H, w); }

// what ns_xg_forward and ns_xg_backward check alike, in this order, and the carved workspace
int common(const std::string& w, const ns_xg_shape* s, const ns_xg_weights* k, const float* tgt, const float* src, const int64_t* lens,
           const uint8_t* keep, float p_drop, const void* saved, const float* attn, void* ws_mem, size_t ws_bytes, Ws* ws) {
  NS_TRY(check_shape(*s, w));
  NS_TRY(check_weights(attn_params(*k), w));
  NS_TRY(check_drop({keep}, p_drop, w));
  NS_TRY(check_aligned(w, {{"tgt", tgt}, {"src", src}, {"saved", saved}, {"attn", attn}, {"the workspace", ws_mem}, {"src_lens", lens, 8}}));
  return carve_checked(carve, counted.abi, *s, ws_mem, ws_bytes, ws, w);
}
}  // namespace

extern "C" int ns_xg_abi_version(void) { return NS_XG_ABI_VERSION; }
extern "C" int ns_xg_last_launches(void) { return t_launches; }

extern "C" size_t ns_xg_ws_bytes(const ns_xg_shape* s) {
  return size_query("ns_xg_ws_bytes", s, check_shape, [](const ns_xg_shape& s, const std::string& w) { return carved_bytes(carve, s, w); });
}

extern "C" size_t ns_xg_saved_bytes(const ns_xg_shape* s) {
  return size_query("ns_xg_saved_bytes", s, check_shape, [](const ns_xg_shape& s, const std::string&) {
    return ((size_t)3 * s.B * s.T * s.d + (size_t)2 * s.B * s.L * s.d) * sizeof(float);
  });
}

extern "C" int ns_xg_kv_splits(const ns_xg_shape* s) {
  const std::string w = "ns_xg_kv_splits: ";
  if (!s) { api_fail(w + "null argument"); return 0; }
  if (check_shape(*s, w)) return 0;
  return xg_kv_splits(s->B, s->H, s->T, s->L);
}

extern "C" int ns_xg_forward(const ns_xg_shape* s, const ns_xg_weights* k, const float* tgt, const float* src, const int64_t* src_lens,
                             const uint8_t* keep, float p_drop, float* y, float* attn, void* saved, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_xg_forward: ";
  t_launches = 0;
  if (!s || !k || !tgt || !src || !src_lens || !y || !attn || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(check_aligned(w, {{"y", y}}));
  Ws ws;
  NS_TRY(common(w, s, k, tgt, src, src_lens, keep, p_drop, saved, attn, ws_mem, ws_bytes, &ws));
  const int MT = s->B * s->T, ML = s->B * s->L, d = s->d, H = s->H, dk = d / H;
  const size_t mt = (size_t)MT * d, ml = (size_t)ML * 2 * d;
  float* q = saved ? (float*)saved : ws.tq;
  float* kv = saved ? q + mt : ws.tkv;
  float* ctx = saved ? kv + ml : ws.c;
  float* z = saved ? ctx + mt : nullptr;
  hipStream_t st = (hipStream_t)stream;
  NS_HIP(launch_xg_pack(XgPack{k->wq, k->wk, k->wv, k->bk, k->bv, k->wfc, ws.wkv, ws.bkv, nullptr, nullptr, nullptr, d}, st));
  ++t_launches;
  NS_TRY(counted.gemm(tgt, k->wq, k->bq, nullptr, q, MT, s->T, d, d, st));
  NS_TRY(counted.gemm(src, ws.wkv, ws.bkv, nullptr, kv, ML, s->L, 2 * d, d, st));
  NS_HIP(launch_cross_attention(q, kv, (const long long*)src_lens, s->B, s->T, s->L, H, dk, ctx, attn, st));
  ++t_launches;
  NS_TRY(counted.gemm(ctx, k->wfc, k->bfc, nullptr, ws.a, MT, s->T, d, d, st));
  NS_HIP(launch_ag_row_forward(ws.a, tgt, keep, 1.f / (1.f - p_drop), k->ln_g, k->ln_b, z, y, MT, d, st));
  ++t_launches;
  return 0;
}

extern "C" int ns_xg_backward(const ns_xg_shape* s, const ns_xg_weights* k, const float* tgt, const float* src, const int64_t* src_lens,
                              const uint8_t* keep, float p_drop, const void* saved, const float* attn, const float* g, const float* dattn,
                              const ns_xg_grads* dg, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_xg_backward: ";
  t_launches = 0;
  if (!s || !k || !tgt || !src || !src_lens || !saved || !attn || !g || !dg || !ws_mem) return api_fail(w + "null argument");
  if (misaligned(g) || misaligned(dattn)) return api_fail(w + "g and dA must be 16-byte aligned");
  std::vector<NamedPtr> outs = attn_params(*dg);
  outs.push_back({"dtgt", dg->dtgt});
  outs.push_back({"dsrc", dg->dsrc});
  bool any = false;
  NS_TRY(check_grads(outs, w, &any));
  Ws ws;
  NS_TRY(common(w, s, k, tgt, src, src_lens, keep, p_drop, saved, attn, ws_mem, ws_bytes, &ws));
  if (!any) return 0;
  const int MT = s->B * s->T, ML = s->B * s->L, d = s->d, H = s->H, dk = d / H, nbt = pg_row_blocks(MT), nbl = pg_row_blocks(ML);
  const size_t mt = (size_t)MT * d, ml = (size_t)ML * 2 * d;
  const float* q = (const float*)saved;
  const float* kv = q + mt;
  const float* ctx = kv + ml;
  const float* z = ctx + mt;
  hipStream_t st = (hipStream_t)stream;
  const bool side_q = dg->dtgt || dg->wq || dg->bq;                       // what reads dQ
  const bool side_kv = dg->dsrc || dg->wk || dg->wv || dg->bk || dg->bv;  // what reads dK | dV
  const bool upstream = side_q || side_kv;                                // anything behind ctx
  PgWgradPlan pt, pl;
  pg_plan_wgrad(MT, d, d, 1, &pt);  // (both accepted by carve above)
  pg_plan_wgrad(ML, d, d, 1, &pl);
  float *dz = ws.a, *du = ws.b, *dctx = ws.c, *dq = ws.tq, *dkv = ws.tkv;
  double* part_row = ws.colq + (size_t)nbt * PG_SLOTS * d;  // stage 1; stage 0 slot 0 holds the column partials of dq

  if (upstream) {
    NS_HIP(launch_xg_pack(XgPack{k->wq, k->wk, k->wv, k->bk, k->bv, k->wfc, nullptr, nullptr, dg->dsrc ? ws.wkvt : nullptr,
                                 dg->dtgt ? ws.wqt : nullptr, ws.wfct, d}, st));
    ++t_launches;
  }
  NS_HIP(launch_ag_row_backward(ag_row_backward_args(MT, d, p_drop, g, z, k->ln_g, keep, dz, du, part_row), st));
  ++t_launches;
  if (dg->wfc) {
    NS_HIP(launch_pg_wgrad(du, ctx, MT, s->T, d, d, 1, pt, ws.partial, dg->wfc, st));
    t_launches += 2;
  }
  if (upstream) {
    NS_TRY(counted.gemm(du, ws.wfct, nullptr, nullptr, dctx, MT, s->T, d, d, st));
    const int nsplit = xg_kv_splits(s->B, H, s->T, s->L);
    NS_HIP(launch_xg_attention_backward(q, kv, ctx, attn, dctx, dattn, (const long long*)src_lens, s->B, s->T, s->L, H, dk, nsplit, ws.stat,
                                        ws.kvpart, dq, side_kv ? dkv : nullptr, st));
    t_launches += 1 + (side_kv ? 1 + (nsplit > 1) : 0);
    if (dg->wq) {
      NS_HIP(launch_pg_wgrad(dq, tgt, MT, s->T, d, d, 1, pt, ws.partial, dg->wq, st));
      t_launches += 2;
    }
    float* dw[2] = {dg->wk, dg->wv};
    for (int i = 0; i < 2; ++i)
      if (dw[i]) {
        NS_HIP(launch_pg_wgrad(dkv + (size_t)i * d, src, ML, s->L, d, d, 1, pl, ws.partial, dw[i], st, 2 * d));
        t_launches += 2;
      }
    if (dg->bq) {
      NS_HIP(launch_pg_colsum(dq, MT, d, 1, ws.colq, st));
      ++t_launches;
    }
    if (dg->bk || dg->bv) {
      NS_HIP(launch_pg_colsum(dkv, ML, d, 2, ws.colkv, st));
      ++t_launches;
    }
    if (dg->dtgt) NS_TRY(counted.gemm(dq, ws.wqt, nullptr, dz, dg->dtgt, MT, s->T, d, d, st));
    if (dg->dsrc) NS_TRY(counted.gemm(dkv, ws.wkvt, nullptr, nullptr, dg->dsrc, ML, s->L, d, 2 * d, st));
  }
  NS_TRY(counted.col_finish(ws.colkv, nbl, d, {dg->bk, dg->bv}, {}, st));
  return counted.col_finish(ws.colq, nbt, d, {dg->bq}, {dg->ln_g, dg->ln_b, dg->bfc}, st);
}

extern "C" int ns_xg_op_attention_backward(const float* q, const float* kv, const float* ctx, const float* attn, const float* dctx,
                                           const float* dattn, const int64_t* src_lens, int B, int T, int L, int d, int H, int kv_splits, float* dq,
                                           float* dkv, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_xg_op_attention_backward: ";
  t_launches = 0;
  if (!q || !kv || !ctx || !attn || !dctx || !src_lens || !dq || !dkv || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(check_dims(B, T, L, d, H, w));
  if (kv_splits < 0 || kv_splits > 8) return api_fail(w + "kv_splits must lie in [0, 8] (0 = the planned number), got " + std::to_string(kv_splits));
  NS_TRY(check_aligned(w, {{"q", q}, {"kv", kv}, {"ctx", ctx}, {"attn", attn}, {"dctx", dctx}, {"dA", dattn}, {"dq", dq}, {"dkv", dkv},
                           {"the workspace", ws_mem}, {"src_lens", src_lens, 8}}));
  const int nsplit = kv_splits ? kv_splits : xg_kv_splits(B, H, T, L);
  Bump bump(ws_mem);
  float* D = bump.f((size_t)B * H * T);
  float* part = nsplit > 1 ? bump.f((size_t)nsplit * B * L * 2 * d) : nullptr;
  if (ws_bytes < bump.off) return api_fail(w + "workspace too small: " + std::to_string(bump.off) + " bytes needed");
  NS_HIP(launch_xg_attention_backward(q, kv, ctx, attn, dctx, dattn, (const long long*)src_lens, B, T, L, H, d / H, nsplit, D, part, dq, dkv,
                                      (hipStream_t)stream));
  t_launches += 2 + (nsplit > 1);
  return 0;
}
