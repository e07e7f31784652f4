// lol_amd/csrc/modswitch_api.cpp — the C ABI of ciphertext modSwitch and multi-hop tunnelling (include/lolhip.h;
// lol-apps SymmSHE.hs:236-246, HomomPRF.hs:153-155, 427-431): host checks, the per-modulus constants (the encoding
// factors are she_host.h's) and the launch plans over k_modswitch (modswitch.hip), lolhip_tunnel_batch and the existing
// transforms.
#include <hip/hip_runtime_api.h>

#include <memory>
#include <vector>

#include "modswitch.h"
#include "she_host.h"

using namespace lolhip;

namespace {

// the bases a side of the internal call may be in.  B_MIXED is what the rescale itself works in and what a tunnel
// hop takes: c_0 in the decoding basis, the other components in the powerful basis
enum Basis { B_POW = 0, B_CRT = 1, B_MIXED = 2 };

// tail's moduli are the last tail.T of all's
bool is_suffix(const std::vector<u64>& all, const std::vector<u64>& tail) {
  if (tail.size() > all.size()) return false;
  const size_t off = all.size() - tail.size();
  for (size_t i = 0; i < tail.size(); ++i)
    if (all[off + i] != tail[i]) return false;
  return true;
}

// d dropped / u added moduli between two plans of one index, or LOLHIP_ERR_INVALID
int relation(const Plan& F, const Plan& G, int* d, int* u) {
  if (F.T < 1 || G.T < 1 || F.T > PIPE_MAX_T || G.T > PIPE_MAX_T || !same_index(F, G)) return LOLHIP_ERR_INVALID;
  *d = *u = 0;
  if (F.T >= G.T) { if (!is_suffix(F.qs, G.qs)) return LOLHIP_ERR_INVALID; *d = F.T - G.T; }
  else { if (!is_suffix(G.qs, F.qs)) return LOLHIP_ERR_INVALID; *u = G.T - F.T; }
  return (*d > MODSW_MAX_D || *u > MODSW_MAX_D) ? LOLHIP_ERR_INVALID : LOLHIP_OK;
}

// every constant of the pass and l' (the statuses of p and of the inverses)
int make_params(const Plan& F, const Plan& G, int d, int u, int enc, int64_t l, int64_t p, ModSwitchParams& mp, u64* l2) {
  if (!p_ok(p)) return LOLHIP_ERR_MODULUS;
  u64 zq[PIPE_MAX_T], zp = 1;
  if (enc == 0) { const int rc = encode_scales(F, p, true, zq, &zp); if (rc) return rc; }      // lsdToMSD
  mp = ModSwitchParams();
  mp.T = F.T; mp.d = d; mp.u = u;
  mp.scaled = (enc == 0 || u > 0) ? 1 : 0;
  for (int t = 0; t < F.T; ++t) {
    const u64 q = F.qs[(size_t)t];
    u64 sc = enc == 0 ? zq[t] : 1 % q;
    for (int a = 0; a < u; ++a) sc = mulmod(sc, G.qs[(size_t)a] % q, q);
    mp.q[t] = q;
    mp.s[t] = sc;
    mp.sp[t] = make_shoup(sc, q).wp;
  }
  for (int i = 0; i < d; ++i)
    for (int t = i + 1; t < F.T; ++t) {
      const u64 q = F.qs[(size_t)t];
      const u64 w = invmod(F.qs[(size_t)i] % q, q);
      if (w == 0) return LOLHIP_ERR_MODULUS;
      mp.inv[i][t] = w;
      mp.invp[i][t] = make_shoup(w, q).wp;
    }
  *l2 = encode_l(l, zp, (u64)p);
  return LOLHIP_OK;
}

struct Switch1 {
  const Plan *F, *G;
  ModSwitchParams mp;
  u64 l2;
};

// the host statuses of one modSwitch, device ones excluded
int prepare(const Plan& F, const Plan& G, int ncs, int in_b, int enc, int64_t l, int64_t p, int out_b, int64_t B,
            Switch1& sw1) {
  if (ncs < 1 || B < 0 || (enc != 0 && enc != 1)) return LOLHIP_ERR_INVALID;
  int d, u;
  int rc = relation(F, G, &d, &u); if (rc) return rc;
  if ((in_b == B_CRT && !F.has_crt) || (out_b == B_CRT && !G.has_crt)) return LOLHIP_ERR_NO_CRT;
  sw1.F = &F; sw1.G = &G;
  return make_params(F, G, d, u, enc, l, p, sw1.mp, &sw1.l2);
}

// the launches of one prepared modSwitch
int run(const Switch1& w, hipStream_t s, const int64_t* cs, int ncs, int in_b, int64_t* out, int out_b, int64_t* work,
        int64_t B) {
  const Plan &F = *w.F, &G = *w.G;
  const i64 slab = B * F.n * F.T;                                     // one component of the input
  const int64_t *in0 = cs, *in = cs;
  // the scale alone (d = u = 0) is per modulus and commutes with the Z_q-linear l / lInv: no trip through the decoding basis
  const bool dec_in = in_b != B_MIXED && !(w.mp.d == 0 && w.mp.u == 0 && out_b != B_MIXED) && !F.prog_linv.stages.empty();
  const bool dec_out = out_b != B_MIXED && !(w.mp.d == 0 && w.mp.u == 0 && in_b != B_MIXED);
  int rc;
  if (in_b == B_CRT) {
    if (hipMemcpyAsync(work, cs, sizeof(int64_t) * (size_t)(ncs * slab), hipMemcpyDeviceToDevice, s) != hipSuccess)
      return LOLHIP_ERR_HIP;
    rc = do_crt(F, s, work, (int64_t)ncs * B, true); if (rc) return rc;
    in0 = in = work;
  }
  if (dec_in) {                                                       // c_0 -> decoding basis (empty for m = 2^k)
    rc = run_prog(F, F.prog_linv, s, work, B, in0 == work ? nullptr : cs); if (rc) return rc;
    in0 = work;
  }
  if (launch_modswitch(s, in0, B * F.n, in, out, (i64)ncs * B * F.n, w.mp) != hipSuccess) return LOLHIP_ERR_HIP;
  if (dec_out) { rc = run_prog_or_copy(G, G.prog_l, s, out, B); if (rc) return rc; }      // empty for m = 2^k
  if (out_b == B_CRT) { rc = do_crt(G, s, out, (int64_t)ncs * B, false); if (rc) return rc; }
  return LOLHIP_OK;
}

int need_both(const lolhip_plan* a, const lolhip_plan* b) {
  const int rc = need_device(a);
  return rc ? rc : need_device(b);
}

}  // namespace

struct lolhip_tunnel_chain {
  int nhops = 0;
  std::vector<const lolhip_ext*> er, es;
  std::vector<const int64_t*> ys, hints;
  std::vector<int> L;                                                // digits of the gadget over each S'
  int64_t base = 0;
  const lolhip_plan *p_in = nullptr, *p_out = nullptr;
  const Plan *first = nullptr, *last = nullptr;                      // R'_0 and the last S' over the up list
  i64 n_max = 0;
};

namespace {

// work (nhops > 0): two ciphertext buffers [2][B][n_max][T_up], the hops ping-pong between them | sub: what the up
// switch, each hop and the down switch carve in turn
struct ChainWork { int64_t *buf[2], *sub; };
ChainWork chain_work(Work& w, const lolhip_tunnel_chain& c, int64_t B) {
  const i64 buf_words = 2 * B * c.n_max * c.first->T;
  ChainWork r = {{w.take(buf_words), w.take(buf_words)}, nullptr};
  const int64_t m = w.mark();
  r.sub = modswitch_work(w, c.p_in->P, 2, B);
  for (int i = 0; i < c.nhops; ++i) {
    w.rewind(m);
    tunnel_work(w, c.er[(size_t)i]->X, c.es[(size_t)i]->X, c.L[(size_t)i], B);
  }
  w.rewind(m);
  modswitch_work(w, *c.last, 2, B);
  return r;
}

}  // namespace

extern "C" {

int64_t lolhip_modswitch_work_len(const lolhip_plan* from, const lolhip_plan* to, int ncs, int64_t B) {
  if (!from || !to || ncs < 1 || B < 0) return LOLHIP_ERR_INVALID;
  int d, u;
  const int rc = relation(from->P, to->P, &d, &u); if (rc) return rc;
  return measure(modswitch_work, from->P, ncs, B);
}

int lolhip_modswitch_batch(const lolhip_plan* from, const lolhip_plan* to, void* stream, const int64_t* cs, int ncs,
                           int cs_crt, int enc, int64_t l, int64_t p, int64_t* out, int out_crt, int64_t* l_out,
                           int64_t* work, int64_t B) {
  if (!from || !to || !l_out) return LOLHIP_ERR_INVALID;
  if (B > 0 && (!cs || !out || !work)) return LOLHIP_ERR_INVALID;
  Switch1 w;
  int rc = prepare(from->P, to->P, ncs, cs_crt ? B_CRT : B_POW, enc, l, p, out_crt ? B_CRT : B_POW, B, w);
  if (rc) return rc;
  rc = need_both(from, to); if (rc) return rc;
  if (B > 0) { rc = run(w, (hipStream_t)stream, cs, ncs, cs_crt ? B_CRT : B_POW, out, out_crt ? B_CRT : B_POW, work, B); if (rc) return rc; }
  *l_out = (int64_t)w.l2;                                             // last: not written where a launch fails
  return LOLHIP_OK;
}

int lolhip_tunnel_chain_create(int nhops, const lolhip_ext* const* x_er, const lolhip_ext* const* x_es,
                               const int64_t* const* ys_crt, const int64_t* const* hints, int64_t base,
                               const lolhip_plan* p_in, const lolhip_plan* p_out, lolhip_tunnel_chain** out) {
  if (!out) return LOLHIP_ERR_INVALID;
  *out = nullptr;
  if (nhops < 0 || !p_in || !p_out || (nhops > 0 && (!x_er || !x_es || !ys_crt || !hints))) return LOLHIP_ERR_INVALID;
  std::unique_ptr<lolhip_tunnel_chain> c(new lolhip_tunnel_chain());
  c->nhops = nhops; c->base = base; c->p_in = p_in; c->p_out = p_out;
  int d, u;
  if (nhops == 0) {
    const int rc = relation(p_in->P, p_out->P, &d, &u); if (rc) return rc;
    *out = c.release();
    return LOLHIP_OK;
  }
  for (int i = 0; i < nhops; ++i) {
    if (!x_er[i] || !x_es[i] || !ys_crt[i] || !hints[i]) return LOLHIP_ERR_INVALID;
    const ExtPlan &ER = x_er[i]->X, &ES = x_es[i]->X;
    // one E' under both, and every hop over the up list (hop 0's moduli)
    if (ER.host.phi != ES.host.phi || ER.lo->qs != ES.lo->qs || ER.hi->qs != x_er[0]->X.hi->qs || ER.hi->T > PIPE_MAX_T)
      return LOLHIP_ERR_INVALID;
    if (i > 0 && !same_index(*x_es[i - 1]->X.hi, *ER.hi)) return LOLHIP_ERR_INVALID;
    DecompParams dp;
    const int rc = make_decomp(*ES.hi, base, dp); if (rc) return rc;
    c->er.push_back(x_er[i]); c->es.push_back(x_es[i]); c->ys.push_back(ys_crt[i]); c->hints.push_back(hints[i]);
    c->L.push_back(dp.L);
    if (ES.hi->n > c->n_max) c->n_max = ES.hi->n;
  }
  c->first = x_er[0]->X.hi;
  c->last = x_es[nhops - 1]->X.hi;
  if (c->first->n > c->n_max) c->n_max = c->first->n;
  int rc = relation(p_in->P, *c->first, &d, &u); if (rc) return rc;
  if (d > 0) return LOLHIP_ERR_INVALID;                              // p_in's moduli are a suffix of the up list
  rc = relation(*c->last, p_out->P, &d, &u); if (rc) return rc;
  if (u > 0) return LOLHIP_ERR_INVALID;
  *out = c.release();
  return LOLHIP_OK;
}

void lolhip_tunnel_chain_destroy(lolhip_tunnel_chain* c) { delete c; }

int64_t lolhip_tunnel_chain_work_len(const lolhip_tunnel_chain* c, int64_t B) {
  if (!c || B < 0) return LOLHIP_ERR_INVALID;
  return c->nhops == 0 ? measure(modswitch_work, c->p_in->P, 2, B) : measure(chain_work, *c, B);
}

int lolhip_tunnel_chain_batch(const lolhip_tunnel_chain* c, void* stream, const int64_t* cs, int cs_crt, int enc,
                              int64_t l, int64_t p, int64_t* out, int out_crt, int64_t* l_out, int64_t* work,
                              int64_t B) {
  if (!c) return LOLHIP_ERR_INVALID;
  if (c->nhops == 0)
    return lolhip_modswitch_batch(c->p_in, c->p_out, stream, cs, 2, cs_crt, enc, l, p, out, out_crt, l_out, work, B);
  if (!l_out || (B > 0 && (!cs || !out || !work))) return LOLHIP_ERR_INVALID;
  // every status first: the up switch (toMSD included), the down switch of an MSD ciphertext, the hops' plans
  Switch1 up, down;
  int rc = prepare(c->p_in->P, *c->first, 2, cs_crt ? B_CRT : B_POW, enc, l, p, B_MIXED, B, up); if (rc) return rc;
  rc = prepare(*c->last, c->p_out->P, 2, B_MIXED, 1, (int64_t)up.l2, p, out_crt ? B_CRT : B_POW, B, down); if (rc) return rc;
  for (int i = 0; i < c->nhops; ++i) {
    const ExtPlan &ER = c->er[(size_t)i]->X, &ES = c->es[(size_t)i]->X;
    if (!ES.hi->has_crt) return LOLHIP_ERR_NO_CRT;
    if (!ER.d_coeffs || !ES.d_embed_pow || !ES.d_embed_dec || !ES.hi->device) return LOLHIP_ERR_NO_DEVICE;
  }
  rc = need_both(c->p_in, c->p_out); if (rc) return rc;
  if (!c->first->device) return LOLHIP_ERR_NO_DEVICE;
  if (B == 0) { *l_out = (int64_t)down.l2; return LOLHIP_OK; }
  hipStream_t s = (hipStream_t)stream;
  Work w(work);
  const auto [buf, sub] = chain_work(w, *c, B);
  rc = run(up, s, cs, 2, cs_crt ? B_CRT : B_POW, buf[0], B_MIXED, sub, B); if (rc) return rc;
  int cur = 0;
  for (int i = 0; i < c->nhops; ++i) {
    const Plan& R = *c->er[(size_t)i]->X.hi;
    const Plan& S = *c->es[(size_t)i]->X.hi;
    const int64_t* c0 = buf[cur];
    rc = lolhip_tunnel_batch(c->er[(size_t)i], c->es[(size_t)i], stream, c0, c0 + B * R.n * R.T, c->ys[(size_t)i],
                             c->hints[(size_t)i], c->base, buf[cur ^ 1], sub, B);
    if (rc) return rc;
    cur ^= 1;
    // back to (decoding, powerful): what the next hop and the rescale take
    rc = do_crt(S, s, buf[cur], 2 * B, true); if (rc) return rc;
    rc = run_prog_or_copy(S, S.prog_linv, s, buf[cur], B); if (rc) return rc;
  }
  rc = run(down, s, buf[cur], 2, B_MIXED, out, out_crt ? B_CRT : B_POW, sub, B); if (rc) return rc;
  *l_out = (int64_t)down.l2;                                          // last: not written where a launch fails
  return LOLHIP_OK;
}

}  // extern "C"
