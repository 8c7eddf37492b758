// srs_contribute.hip -- one powers-of-tau contribution (g16_srs_contribute): the point arithmetic of `snarkjs
// powersoftau contribute` (and, from the string of generators, of `powersoftau new`).  The string of
// (tau, alpha, beta) becomes the string of (tau t, alpha a, beta b):
//   tau_g1[i], tau_g2[i] times t^i, alpha_tau_g1[i] times a t^i, beta_tau_g1[i] times b t^i, beta_g2 times b.
// The section-7 transcript of a .ptau is NOT handled (include/g16_amd.h).
//
// Unlike contribute.hip's one shared d^-1, EVERY point has its own full-width scalar, so there is no wave-uniform
// digit schedule to recode on the host.  Per chunk of `chunk` points of one array, starting at power `base`:
//   k_sx_scalars  lane i: c t^(base + i) as a canonical 256-bit integer, from t^(2^j) (24 squarings, on the host,
//                 once per call) and the chunk's c t^base (one entry per chunk, computed on the host up front).
//                 No host loop over points.
//   k_sx_mul<F>   one lane per point, F = Fq (G1) or Fq2 (G2): 256 bit positions, the same for every lane; a
//                 doubling at each, and a MIXED addition of P (8M + 2S, P stays affine in registers) predicated on
//                 the lane's own bit.  A per-lane signed-digit recoding would buy nothing: a wave pays for the
//                 addition whenever ANY of its 64 lanes has a non-zero digit, which is almost every position.  The
//                 scalar is read from memory one word per 32 positions: a register array indexed by the loop
//                 counter would be scratch.  A lane at infinity, or above the leading bit of its scalar, idles.
//   k_xyzz_to_affine<F>  (toaffine.h) back to canonical affine with ONE inversion per run of 8 points
//                 (Montgomery's trick down each lane's run), in place of the chunk's input points.
// Two page-locked host slots and two device slots; chunk k + 1 is staged and copied while the kernels of chunk k
// run, and the results of chunk k come back on a third stream under the kernels of chunk k + 1.
#include <stdlib.h>

#include "keycheck.h"
#include "ntt.h"
#include "toaffine.h"

namespace g16 {
namespace {

constexpr uint32_t SX_DEFAULT_CHUNK = 1u << 18;
constexpr int SX_POW_BITS = 24;  // t^(2^j), j < 24: a lane's index within a chunk is below 2^24 (chunk_from_env)

enum { T_UPLOAD = 0, T_SCALARS, T_MUL_G1, T_MUL_G2, T_AFFINE, T_DOWNLOAD, T_COUNT };
thread_local PhaseTimes<T_COUNT> t_phase;

// out[i] = scale * t^i, canonical; tab[j] = t^(2^j)
__global__ void __launch_bounds__(256) k_sx_scalars(const Fr* tab, const Fr* scale, uint32_t n, U256* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr r = *scale;
#pragma unroll 1
  for (int j = 0; j < SX_POW_BITS; ++j)
    if ((i >> j) & 1) r = r * tab[j];
  out[i] = r.to_canonical();
}

template <class F>
__global__ void __launch_bounds__(KC_BLOCK) k_sx_mul(const Affine<F>* pts, const U256* sc, uint32_t n, XYZZ<F>* work) {
  const uint32_t i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const Affine<F> p = pts[i];
  const uint32_t* k = sc[i].v;
  XYZZ<F> acc = XYZZ<F>::infinity();
#pragma unroll 1
  for (int w = 7; w >= 0; --w) {
    uint32_t kw = k[w];
#pragma unroll 1
    for (int b = 0; b < 32; ++b, kw <<= 1) {
      acc.dbl_in_place();
      if (kw >> 31) acc.madd(p);
    }
  }
  work[i] = acc;
}

struct Item {
  bool g2;
  const uint8_t* src;
  uint8_t* dst;
  uint32_t count;
};

// the events of one slot, in the order they complete
enum { E_UP0 = 0, E_UP1, E_C0, E_C1, E_C2, E_C3, E_DN0, E_DN1, E_COUNT };

// t, a, b and everything derived from them on the host: wiped on every way out
struct Secret {
  Fr s[3];  // t, a, b
  U256 c;
  FrPool pool;  // the candidates of drawn secrets
  std::vector<Fr> dev;  // what goes to the device: t^(2^j), j < SX_POW_BITS, then one c t^base per chunk
  ~Secret() {
    if (!dev.empty()) wipe(dev.data(), dev.size() * sizeof(Fr));
    wipe(s, sizeof s);
    wipe(&c, sizeof c);
  }
};

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" g16_status g16_srs_contribute(int device, const g16_srs_desc* srs, const uint64_t* secrets,
                                         uint8_t* tau_g1_out, uint8_t* tau_g2_out, uint8_t* alpha_tau_g1_out,
                                         uint8_t* beta_tau_g1_out, uint8_t beta_g2_out[128]) {
  if (!srs || !tau_g1_out || !tau_g2_out || !alpha_tau_g1_out || !beta_tau_g1_out || !beta_g2_out) return G16_ERR_INVALID;
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return G16_ERR_INVALID;
  const uint64_t n1 = srs->n_tau_g1, n2 = srs->n_tau;
  if (n1 == 0 || n2 == 0) return G16_ERR_INVALID;
  Secret sec;
  if (secrets) {
    memcpy(sec.s, secrets, sizeof sec.s);
    for (const Fr& x : sec.s)
      if (!fr_words_canonical(x) || x.is_zero()) return G16_ERR_INVALID;
  }
  if (const g16_status ds = device_ok(device)) return ds;
  if (!secrets)
    for (Fr& x : sec.s)
      if (!sec.pool.draw_fr(&x, true)) return G16_ERR_INTERNAL;  // never a fixed fallback
  const Fr &t = sec.s[0], &a = sec.s[1], &b = sec.s[2];

  return guarded_call([&]() -> g16_status {
    const uint32_t chunk = chunk_from_env("G16_SRSCONTRIB_CHUNK", SX_DEFAULT_CHUNK, n1 > n2 ? n1 : n2);

    // the chunks of the four arrays, and per chunk its c t^base behind the powers t^(2^j)
    std::vector<Item> items;
    sec.dev.reserve(SX_POW_BITS + 4 + (n1 + 3 * n2) / chunk);  // no reallocation: no unwiped copy left behind
    {
      Fr x = t;
      for (int j = 0; j < SX_POW_BITS; ++j) {
        sec.dev.push_back(x);
        x = x.sqr();
      }
      wipe(&x, sizeof x);
    }
    auto add_items = [&](bool g2, const Fr& c, const uint8_t* src, uint8_t* dst, uint64_t total) {
      const size_t w = g2 ? 128 : 64;
      for (uint64_t at = 0; at < total; at += chunk) {
        items.push_back(Item{g2, src + at * w, dst + at * w, (uint32_t)(total - at < chunk ? total - at : chunk)});
        sec.dev.push_back(c * fr_pow_u64(t, at));
      }
    };
    add_items(false, Fr::one(), srs->tau_g1, tau_g1_out, n1);
    add_items(false, a, srs->alpha_tau_g1, alpha_tau_g1_out, n2);
    add_items(false, b, srs->beta_tau_g1, beta_tau_g1_out, n2);
    add_items(true, Fr::one(), srs->tau_g2, tau_g2_out, n2);

    // beta_g2: one point, on the host with the same field classes
    G2Affine bg2;
    memcpy(&bg2, srs->beta_g2, 128);
    sec.c = b.to_canonical();
    const G2Affine nbg2 = G2XYZZ::from_affine(bg2).mul(sec.c).to_affine();

    G16_HIP(hipSetDevice(device));
    // every allocation of the call: nothing is allocated inside the chunk loop
    const size_t slot_bytes = (size_t)chunk * 128;
    PinnedBuf pin[2];
    DevBuf<uint8_t> dslot[2];
    DevBuf<uint8_t> dwork;  // chunk x G2XYZZ; the G1 chunks use the front half
    DevBuf<U256> dsc;
    DevBuf<Fr> dsec;
    StreamBox copy, comp, down;
    EventBox ev[2][E_COUNT];
    for (int s = 0; s < 2; ++s) {
      pin[s].alloc(slot_bytes);
      dslot[s].alloc(slot_bytes);
      for (int e = 0; e < E_COUNT; ++e) ev[s][e].create(true);
    }
    dwork.alloc((size_t)chunk * sizeof(G2XYZZ));
    dsc.alloc(chunk);
    dsec.alloc(sec.dev.size());
    copy.create();
    comp.create();
    down.create();
    G16_HIP(hipMemcpy(dsec.p, sec.dev.data(), sec.dev.size() * sizeof(Fr), hipMemcpyHostToDevice));

    PhaseTimes<T_COUNT> ms{};  // of this call: the chunks add up, the thread's values change when all is done
    auto collect = [&](int s, bool g2) {
      ms.take(Stored::ADD, ev[s],
              {{E_UP0, E_UP1, T_UPLOAD},
               {E_C0, E_C1, T_SCALARS},
               {E_C1, E_C2, g2 ? T_MUL_G2 : T_MUL_G1},
               {E_C2, E_C3, T_AFFINE},
               {E_DN0, E_DN1, T_DOWNLOAD}});
    };

    for (size_t k = 0; k < items.size() + 2; ++k) {
      const int s = (int)(k & 1);
      if (k >= 2) {  // the results of the chunk that used this slot two chunks ago
        const Item& was = items[k - 2];
        G16_HIP(hipEventSynchronize(ev[s][E_DN1].e));
        memcpy(was.dst, pin[s].p, (size_t)was.count * (was.g2 ? 128 : 64));
        collect(s, was.g2);
      }
      if (k >= items.size()) continue;
      const Item& it = items[k];
      const uint32_t n = it.count;
      const size_t bytes = (size_t)n * (it.g2 ? 128 : 64);
      uint8_t* dv = dslot[s].p;
      memcpy(pin[s].p, it.src, bytes);
      G16_LAUNCH(k_phase_mark<>, 1, 1, 0, copy.s);
      G16_HIP(hipEventRecord(ev[s][E_UP0].e, copy.s));
      G16_HIP(hipMemcpyAsync(dv, pin[s].p, bytes, hipMemcpyHostToDevice, copy.s));
      G16_HIP(hipEventRecord(ev[s][E_UP1].e, copy.s));
      G16_HIP(hipStreamWaitEvent(comp.s, ev[s][E_UP1].e, 0));
      G16_LAUNCH(k_phase_mark<>, 1, 1, 0, comp.s);
      G16_HIP(hipEventRecord(ev[s][E_C0].e, comp.s));
      G16_LAUNCH(k_sx_scalars, ceil_div(n, 256), 256, 0, comp.s, (const Fr*)dsec.p,
                 (const Fr*)(dsec.p + SX_POW_BITS + k), n, dsc.p);
      G16_HIP(hipEventRecord(ev[s][E_C1].e, comp.s));
      if (it.g2) {
        G16_LAUNCH((k_sx_mul<Fq2>), ceil_div(n, KC_BLOCK), KC_BLOCK, 0, comp.s, (const G2Affine*)dv, (const U256*)dsc.p,
                   n, (G2XYZZ*)dwork.p);
        G16_HIP(hipEventRecord(ev[s][E_C2].e, comp.s));
        xyzz_to_affine<Fq2>((const G2XYZZ*)dwork.p, n, (G2Affine*)dv, comp.s);
      } else {
        G16_LAUNCH((k_sx_mul<Fq>), ceil_div(n, KC_BLOCK), KC_BLOCK, 0, comp.s, (const G1Affine*)dv, (const U256*)dsc.p,
                   n, (G1XYZZ*)dwork.p);
        G16_HIP(hipEventRecord(ev[s][E_C2].e, comp.s));
        xyzz_to_affine<Fq>((const G1XYZZ*)dwork.p, n, (G1Affine*)dv, comp.s);
      }
      G16_HIP(hipEventRecord(ev[s][E_C3].e, comp.s));
      G16_HIP(hipStreamWaitEvent(down.s, ev[s][E_C3].e, 0));
      G16_LAUNCH(k_phase_mark<>, 1, 1, 0, down.s);
      G16_HIP(hipEventRecord(ev[s][E_DN0].e, down.s));
      G16_HIP(hipMemcpyAsync(pin[s].p, dv, bytes, hipMemcpyDeviceToHost, down.s));
      G16_HIP(hipEventRecord(ev[s][E_DN1].e, down.s));
    }
    // nothing derived from the secrets outlives the call on the device
    G16_HIP(hipMemsetAsync(dsec.p, 0, dsec.bytes(), comp.s));
    G16_HIP(hipMemsetAsync(dsc.p, 0, dsc.bytes(), comp.s));
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(comp.s));
    G16_HIP(hipStreamSynchronize(down.s));
    memcpy(beta_g2_out, &nbg2, 128);
    t_phase = ms;
    return G16_OK;
  });
}

extern "C" g16_status g16_srs_contribute_times(float* ms, uint32_t cap) {
  return t_phase.read(ms, cap);
}
