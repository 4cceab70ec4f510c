// Length-aware LSTM recurrence: the kernels of lstm.hip for zero-padded clips of unequal length
// (lens [B], int, device memory; clamped here to [0, T]).  The semantics are those of
// pack_padded_sequence -> nn.LSTM -> pad_packed_sequence(total_length = T): for clip b with
// L = lens[b], out[b][t] is h_t for t < L and zero for t >= L, h_n / c_n are the state after step
// L - 1 (zero for L = 0); the backward ignores dout[b][t >= L], takes dh_n / dc_n in at step L - 1
// and writes zero pre-activation gradients for t >= L, so the clip adds nothing to any gradient
// from its padding and dx[b][t >= L] is exactly zero.
//
// Three kernel families, each the arithmetic of its fixed-length namesake in lstm.hip, expression
// for expression (with lens[b] = T the results are bit-identical to xcp_lstm_fwd / xcp_lstm_bwd):
//   register-resident (H = 64 / 128): one workgroup per clip, L is workgroup-uniform; the
//     workgroup walks its clip's L steps, zero-fills its tail rows with 16-B stores from all 1024
//     threads and leaves;
//   per-step (H = 256 / 512 / 1024, B <= 32): the (clip, unit) cell threads are masked per clip;
//   generic (any other shape, kernel = 1): as the register-resident pair.
// They are separate kernels, not instantiations shared with lstm.hip, so the fixed-length entry
// points execute exactly the code they did before this file existed.  The price is that the
// compiler contracts each copy on its own: where it chose differently (one product in the per-step
// backward's cell) the rounding is spelled out here, and tests/test_gpu_lstm_varlen.py pins the
// bit-identity per family.
//
// A length-aware call never takes the persistent, gather or clip-grouped kernels of lstm.hip:
// H = 256 / 512 go to the per-step kernels here.  Those three hand steps over through polled
// counters with a timeout (the open findings in ADVICE.md); nothing here polls, counts or can time
// out, so this file does not widen them.  A persistent length-aware form is not written.
//
// Saved state for t >= L: hprev is written (zero) because the weight gradient dW_hh = dgates^T hprev
// runs over all B*T rows and 0 x (uninitialised) may be NaN; cst and gates are left unwritten there
// and no kernel below uses a value loaded from such a row (the per-step kernels load some as
// stand-in addresses and select them away, as lstm.hip does for absent operands).
#include "common.h"

namespace {

XCP_DEV float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// 1 - v * v with the product rounded before the subtraction (no fma contraction)
XCP_DEV float one_minus_sq_unfused(float v) {
#pragma clang fp contract(off)
  const float p = v * v;
  return 1.f - p;
}

XCP_DEV int vl_len(const int* __restrict__ lens, int b, int T) { return min(max(lens[b], 0), T); }

// ---------------------------------------------------------------------------------
// generic pair (lstm_fwd_kernel / lstm_bwd_kernel of lstm.hip)
__global__ __launch_bounds__(256) void lstm_fwd_vl_kernel(const float* __restrict__ xproj, const float* __restrict__ whhT,
                                                          const float* __restrict__ bih, const float* __restrict__ bhh,
                                                          float* __restrict__ out, float* __restrict__ hprev,
                                                          float* __restrict__ cst, float* __restrict__ gates,
                                                          float* __restrict__ hn, float* __restrict__ cn,
                                                          const int* __restrict__ lens, int T, int H) {
  extern __shared__ float sm[];   // h [H], c [H], gate pre-activations [4H]
  float* sh = sm;
  float* sc = sm + H;
  float* sg = sm + 2 * H;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int G4 = 4 * H;
  const int L = vl_len(lens, b, T);
  for (int k = tid; k < H; k += blockDim.x) { sh[k] = 0.f; sc[k] = 0.f; }
  __syncthreads();
  for (int t = 0; t < L; ++t) {
    const float* xp = xproj + ((long)b * T + t) * G4;
    for (int j = tid; j < G4; j += blockDim.x) {
      float acc = xp[j] + bih[j] + bhh[j];
      for (int k = 0; k < H; ++k) acc = fmaf(sh[k], whhT[(long)k * G4 + j], acc);
      sg[j] = acc;
    }
    __syncthreads();
    float* gt = gates + ((long)b * T + t) * G4;
    const long ob = ((long)b * T + t) * H;
    for (int k = tid; k < H; k += blockDim.x) {
      const float ig = sigm(sg[k]), fg = sigm(sg[H + k]), gg = tanhf(sg[2 * H + k]), og = sigm(sg[3 * H + k]);
      const float c = fmaf(fg, sc[k], ig * gg);
      const float h = og * tanhf(c);
      gt[k] = ig; gt[H + k] = fg; gt[2 * H + k] = gg; gt[3 * H + k] = og;
      hprev[ob + k] = sh[k];
      cst[ob + k] = c;
      out[ob + k] = h;
    }
    __syncthreads();
    for (int k = tid; k < H; k += blockDim.x) {
      sh[k] = out[ob + k];
      sc[k] = cst[ob + k];
    }
    __syncthreads();
  }
  for (int k = tid; k < H; k += blockDim.x) {
    hn[(long)b * H + k] = sh[k];
    cn[(long)b * H + k] = sc[k];
  }
  // tail rows t >= L (contiguous): out and hprev zero (H is arbitrary here: 4-B stores)
  const long tb = ((long)b * T + L) * H, tn = (long)(T - L) * H;
  for (long e = tid; e < tn; e += blockDim.x) {
    out[tb + e] = 0.f;
    hprev[tb + e] = 0.f;
  }
}

__global__ __launch_bounds__(256) void lstm_bwd_vl_kernel(const float* __restrict__ dout, const float* __restrict__ dhn,
                                                          const float* __restrict__ dcn, const float* __restrict__ whh,
                                                          const float* __restrict__ cst, const float* __restrict__ gates,
                                                          float* __restrict__ dgates, const int* __restrict__ lens, int T,
                                                          int H) {
  extern __shared__ float sm[];   // dh [H], dc [H], dgates_t [4H]
  float* sdh = sm;
  float* sdc = sm + H;
  float* sdg = sm + 2 * H;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int G4 = 4 * H;
  const int L = vl_len(lens, b, T);
  for (int k = tid; k < H; k += blockDim.x) {
    sdh[k] = dhn ? dhn[(long)b * H + k] : 0.f;
    sdc[k] = dcn ? dcn[(long)b * H + k] : 0.f;
  }
  __syncthreads();
  for (int t = L - 1; t >= 0; --t) {
    const long ob = ((long)b * T + t) * H;
    const float* gt = gates + ((long)b * T + t) * G4;
    float* dg = dgates + ((long)b * T + t) * G4;
    for (int k = tid; k < H; k += blockDim.x) {
      const float dh = sdh[k] + (dout ? dout[ob + k] : 0.f);
      const float c = cst[ob + k];
      const float cp = t > 0 ? cst[ob - H + k] : 0.f;
      const float ig = gt[k], fg = gt[H + k], gg = gt[2 * H + k], og = gt[3 * H + k];
      const float tc = tanhf(c);
      const float dO = dh * tc;
      const float dc = sdc[k] + dh * og * (1.f - tc * tc);
      const float dI = dc * gg, dG = dc * ig, dF = dc * cp;
      sdc[k] = dc * fg;
      const float a0 = dI * ig * (1.f - ig), a1 = dF * fg * (1.f - fg), a2 = dG * (1.f - gg * gg),
                  a3 = dO * og * (1.f - og);
      sdg[k] = a0; sdg[H + k] = a1; sdg[2 * H + k] = a2; sdg[3 * H + k] = a3;
      dg[k] = a0; dg[H + k] = a1; dg[2 * H + k] = a2; dg[3 * H + k] = a3;
    }
    __syncthreads();
    // dh_{t-1}[k] = sum_j dgates[j] * whh[j][k]
    for (int k = tid; k < H; k += blockDim.x) {
      float acc = 0.f;
      for (int j = 0; j < G4; ++j) acc = fmaf(sdg[j], whh[(long)j * H + k], acc);
      sdh[k] = acc;
    }
    __syncthreads();
  }
  // tail rows t >= L: zero pre-activation gradients
  const long tb = ((long)b * T + L) * G4, tn = (long)(T - L) * G4;
  for (long e = tid; e < tn; e += blockDim.x) dgates[tb + e] = 0.f;
}


// ---------------------------------------------------------------------------------
// register-resident pair (lstm_fwd_reg_kernel / lstm_bwd_reg_kernel of lstm.hip): thread layout, LDS
// layout and every expression as there; the step loops stop at the clip's own length.
template <int H>
__global__ __launch_bounds__(1024) void lstm_fwd_reg_vl_kernel(const float* __restrict__ xproj,
                                                               const float* __restrict__ whh,
                                                               const float* __restrict__ bih,
                                                               const float* __restrict__ bhh, float* __restrict__ out,
                                                               float* __restrict__ hprev, float* __restrict__ cst,
                                                               float* __restrict__ gates, float* __restrict__ hn,
                                                               float* __restrict__ cn, const int* __restrict__ lens,
                                                               int T) {
  constexpr int G4 = 4 * H, S = 1024 / G4, KPT = H / S, PADK = KPT + 4;
  static_assert(S >= 1 && KPT % 4 == 0, "unsupported H");
  __shared__ __attribute__((aligned(16))) float sh[S * PADK];   // h_{t-1}, part s at s*PADK (bank-spread)
  __shared__ float sg[G4];                                      // activated gates of step t
  const int tid = threadIdx.x, b = blockIdx.x;
  const int L = vl_len(lens, b, T);   // workgroup-uniform
  const int j = tid / S, s = tid % S;
  float w[KPT];
  const float* wp = whh + (long)j * H + s * KPT;
#pragma unroll
  for (int q = 0; q < KPT; q += 4) {
    const float4 v = *reinterpret_cast<const float4*>(wp + q);
    w[q] = v.x; w[q + 1] = v.y; w[q + 2] = v.z; w[q + 3] = v.w;
  }
  const float bias = bih[j] + bhh[j];
  const bool gate_tanh = (j / H) == 2;
  auto hidx = [](int k) { return (k / KPT) * PADK + k % KPT; };
  if (tid < H) sh[hidx(tid)] = 0.f;
  float c = 0.f;                                 // c_{t-1}[tid] for tid < H
  const float* xb = xproj + (long)b * T * G4;
  float xn = s == 0 ? xb[j] : 0.f;               // (row 0 exists for L = 0 too: T >= 1)
  __syncthreads();
  for (int t = 0; t < L; ++t) {
    const float xc = xn;
    if (s == 0 && t + 1 < L) xn = xb[(long)(t + 1) * G4 + j];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    const float* hp = sh + s * PADK;
#pragma unroll
    for (int q = 0; q < KPT; q += 4) {
      const float4 h4 = *reinterpret_cast<const float4*>(hp + q);
      a0 = fmaf(h4.x, w[q], a0);
      a1 = fmaf(h4.y, w[q + 1], a1);
      a2 = fmaf(h4.z, w[q + 2], a2);
      a3 = fmaf(h4.w, w[q + 3], a3);
    }
    float acc = (a0 + a1) + (a2 + a3);
#pragma unroll
    for (int o = 1; o < S; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (s == 0) {
      const float pre = acc + xc + bias;
      const float v = gate_tanh ? tanhf(pre) : sigm(pre);
      sg[j] = v;
      gates[((long)b * T + t) * G4 + j] = v;
    }
    __syncthreads();
    if (tid < H) {
      const long ob = ((long)b * T + t) * H + tid;
      const float ig = sg[tid], fg = sg[H + tid], gg = sg[2 * H + tid], og = sg[3 * H + tid];
      hprev[ob] = sh[hidx(tid)];
      c = fmaf(fg, c, ig * gg);
      const float h = og * tanhf(c);
      cst[ob] = c;
      out[ob] = h;
      sh[hidx(tid)] = h;      // every read of h_{t-1} happened before the barrier above
    }
    __syncthreads();
  }
  if (tid < H) {
    hn[(long)b * H + tid] = sh[hidx(tid)];
    cn[(long)b * H + tid] = c;
  }
  // tail rows t >= L, contiguous from row b*T + L (a multiple of H floats: 16-B aligned): out and
  // hprev zero, one float4 per thread and pass
  const long n4 = (long)(T - L) * (H / 4);
  float4* po = reinterpret_cast<float4*>(out + ((long)b * T + L) * H);
  float4* ph = reinterpret_cast<float4*>(hprev + ((long)b * T + L) * H);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long e = tid; e < n4; e += 1024) {
    po[e] = z;
    ph[e] = z;
  }
}

template <int H>
__global__ __launch_bounds__(1024) void lstm_bwd_reg_vl_kernel(const float* __restrict__ dout,
                                                               const float* __restrict__ dhn,
                                                               const float* __restrict__ dcn,
                                                               const float* __restrict__ whh,
                                                               const float* __restrict__ cst,
                                                               const float* __restrict__ gates,
                                                               float* __restrict__ dgates,
                                                               const int* __restrict__ lens, int T) {
  constexpr int G4 = 4 * H, P = 1024 / H, JPT = G4 / P, PADJ = JPT + 4;
  static_assert(P >= 1 && JPT % 4 == 0, "unsupported H");
  __shared__ __attribute__((aligned(16))) float sdg[P * PADJ];
  __shared__ float sdh[H];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int L = vl_len(lens, b, T);   // workgroup-uniform
  const int k = tid / P, p = tid % P;
  float w[JPT];
#pragma unroll
  for (int q = 0; q < JPT; ++q) w[q] = whh[(long)(p * JPT + q) * H + k];
  auto gidx = [](int jj) { return (jj / JPT) * PADJ + jj % JPT; };
  float dc = 0.f;                                // dc carried into step t, unit tid < H
  // per-step inputs of unit tid, prefetched one step ahead
  float n_c = 0.f, n_cp = 0.f, n_i = 0.f, n_f = 0.f, n_g = 0.f, n_o = 0.f, n_do = 0.f;
  auto fetch = [&](int t) {
    const long ob = ((long)b * T + t) * H + tid;
    const float* gt = gates + ((long)b * T + t) * G4;
    n_c = cst[ob];
    n_cp = t > 0 ? cst[ob - H] : 0.f;
    n_i = gt[tid]; n_f = gt[H + tid]; n_g = gt[2 * H + tid]; n_o = gt[3 * H + tid];
    n_do = dout ? dout[ob] : 0.f;
  };
  if (tid < H) {
    sdh[tid] = dhn ? dhn[(long)b * H + tid] : 0.f;
    dc = dcn ? dcn[(long)b * H + tid] : 0.f;
    if (L > 0) fetch(L - 1);
  }
  __syncthreads();
  for (int t = L - 1; t >= 0; --t) {
    if (tid < H) {
      const float c = n_c, cp = n_cp, ig = n_i, fg = n_f, gg = n_g, og = n_o;
      const float dh = sdh[tid] + n_do;
      if (t > 0) fetch(t - 1);
      const float tc = tanhf(c);
      const float dO = dh * tc;
      const float dct = dc + dh * og * (1.f - tc * tc);
      const float dI = dct * gg, dG = dct * ig, dF = dct * cp;
      dc = dct * fg;
      const float g0 = dI * ig * (1.f - ig), g1 = dF * fg * (1.f - fg), g2 = dG * (1.f - gg * gg),
                  g3 = dO * og * (1.f - og);
      float* dg = dgates + ((long)b * T + t) * G4;
      dg[tid] = g0; dg[H + tid] = g1; dg[2 * H + tid] = g2; dg[3 * H + tid] = g3;
      sdg[gidx(tid)] = g0; sdg[gidx(H + tid)] = g1; sdg[gidx(2 * H + tid)] = g2; sdg[gidx(3 * H + tid)] = g3;
    }
    __syncthreads();
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    const float* gp = sdg + p * PADJ;
#pragma unroll
    for (int q = 0; q < JPT; q += 4) {
      const float4 g4 = *reinterpret_cast<const float4*>(gp + q);
      a0 = fmaf(g4.x, w[q], a0);
      a1 = fmaf(g4.y, w[q + 1], a1);
      a2 = fmaf(g4.z, w[q + 2], a2);
      a3 = fmaf(g4.w, w[q + 3], a3);
    }
    float acc = (a0 + a1) + (a2 + a3);
#pragma unroll
    for (int o = 1; o < P; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (p == 0) sdh[k] = acc;
    __syncthreads();
  }
  // tail rows t >= L (contiguous, 16-B aligned): zero pre-activation gradients
  const long n4 = (long)(T - L) * (G4 / 4);
  float4* pd = reinterpret_cast<float4*>(dgates + ((long)b * T + L) * G4);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long e = tid; e < n4; e += 1024) pd[e] = z;
}


// ---------------------------------------------------------------------------------
// per-step pair (lstm_fwd_step_kernel / lstm_bwd_step_kernel of lstm.hip): one launch per time step
// over H / 2 workgroups.  Every dot product runs for every clip as there (a finished clip's
// h_{t-1} / dgates_{t+1} row is the zero this pair wrote, or the clip's last real row at t = L:
// finite either way, and nothing of that clip is read again); only the (clip, unit) cell threads look
// at the clip's length.
constexpr int LS_UPW = 2;              // hidden units per workgroup
constexpr int LS_MAXB = 32;            // clips (register partials per thread)

template <int KS>   // KS = H / 32 (k values per slice)
__global__ __launch_bounds__(256) void lstm_fwd_step_vl_kernel(const float* __restrict__ xproj, const float* __restrict__ whh,
                                                               const float* __restrict__ bih, const float* __restrict__ bhh,
                                                               float* __restrict__ out, float* __restrict__ hprev,
                                                               float* __restrict__ cst, float* __restrict__ gates,
                                                               float* __restrict__ hn, float* __restrict__ cn,
                                                               const int* __restrict__ lens, int B, int T, int t) {
  constexpr int H = KS * 32, G4 = 4 * H, PS = KS + 4;   // LDS slice pitch (floats)
  constexpr int RP = 33;                                // pitch of a (row, clip) partial row
  extern __shared__ float sm[];   // h_{t-1} [B][32][PS] (then the partials [8][B][RP]), then pre [8][B]
  float* sh = sm;
  float* spre = sm + B * 32 * PS;
  const int tid = threadIdx.x, u0 = blockIdx.x * LS_UPW;
  const int r = tid >> 5, s = tid & 31, q = r >> 1, uu = r & 1;
  const int j = q * H + u0 + uu;
  float w[KS];
#pragma unroll
  for (int i = 0; i < KS; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(whh + (long)j * H + s * KS + i);
    w[i] = v.x; w[i + 1] = v.y; w[i + 2] = v.z; w[i + 3] = v.w;
  }
  // stage h_{t-1} (zero at t = 0): unconditional clamped loads, selected away at t = 0
  const int n4 = B * H / 4;
  const int tp = t > 0 ? t - 1 : 0;
  for (int e0 = tid; e0 < n4; e0 += 8 * 256) {
    float4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = min(e0 + i * 256, n4 - 1);
      const int b = e / (H / 4), k4 = (e - b * (H / 4)) * 4;
      v[i] = *reinterpret_cast<const float4*>(out + ((long)b * T + tp) * H + k4);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = e0 + i * 256;
      const int b = e / (H / 4), k4 = (e - b * (H / 4)) * 4;
      if (e < n4)
        *reinterpret_cast<float4*>(sh + (b * 32 + k4 / KS) * PS + (k4 % KS)) =
            t > 0 ? v[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __syncthreads();
  float acc[LS_MAXB];
#pragma unroll
  for (int b = 0; b < LS_MAXB; ++b) {
    acc[b] = 0.f;
    if (b < B) {
      const float4* hb = reinterpret_cast<const float4*>(sh + (b * 32 + s) * PS);
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int i = 0; i < KS; i += 4) {
        const float4 h4 = hb[i / 4];
        a0 = fmaf(w[i], h4.x, a0);
        a1 = fmaf(w[i + 1], h4.y, a1);
        a0 = fmaf(w[i + 2], h4.z, a0);
        a1 = fmaf(w[i + 3], h4.w, a1);
      }
      acc[b] = a0 + a1;
    }
  }
  __syncthreads();   // h_{t-1} no longer read: its space takes the partials
  float* red = sm;
#pragma unroll
  for (int b = 0; b < LS_MAXB; ++b)
    if (b < B) red[(r * B + b) * RP + s] = acc[b];
  __syncthreads();
  if (tid < 8 * B) {
    const float* pr = red + tid * RP;
    float v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = pr[i];
#pragma unroll
    for (int w2 = 1; w2 < 32; w2 <<= 1)
#pragma unroll
      for (int i = 0; i < 32; i += 2 * w2) v[i] = v[i] + v[i + w2];
    spre[tid] = v[0];   // tid = row * B + clip
  }
  __syncthreads();
  if (tid < B * LS_UPW) {
    const int b = tid / LS_UPW, v = tid - b * LS_UPW, k = u0 + v;
    const int L = vl_len(lens, b, T);
    const bool live = t < L;
    const float* xp = xproj + ((long)b * T + t) * G4;
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int jj = g * H + k;
      pre[g] = spre[(g * 2 + v) * B + b] + xp[jj] + bih[jj] + bhh[jj];
    }
    const float ig = sigm(pre[0]), fg = sigm(pre[1]), gg = tanhf(pre[2]), og = sigm(pre[3]);
    const long ob = ((long)b * T + t) * H;
    const long op = t > 0 ? ob - H + k : ob + k;   // t = 0: a valid stand-in, selected away
    // (t > L: row t - 1 of cst was never written -- a valid address whose value is selected away)
    const float vcp = cst[op], vhp = out[op];
    const float cp = t > 0 ? vcp : 0.f;
    const float c = fmaf(fg, cp, ig * gg);
    const float h = og * tanhf(c);
    // past the clip's end: zero out / hprev, no state, no saved gates
    hprev[ob + k] = live && t > 0 ? vhp : 0.f;
    out[ob + k] = live ? h : 0.f;
    if (live) {
      float* gt = gates + ((long)b * T + t) * G4;
      gt[k] = ig; gt[H + k] = fg; gt[2 * H + k] = gg; gt[3 * H + k] = og;
      cst[ob + k] = c;
    }
    if (t == L - 1) {
      hn[(long)b * H + k] = h;
      cn[(long)b * H + k] = c;
    }
    if (t == 0 && L == 0) {
      hn[(long)b * H + k] = 0.f;
      cn[(long)b * H + k] = 0.f;
    }
  }
}

// whhT[k][j] = whh[j][k] (once per backward call, so a workgroup's W_hh columns are rows)
__global__ __launch_bounds__(256) void lstm_transpose_vl_kernel(const float* __restrict__ whh, float* __restrict__ whhT,
                                                                int H) {
  __shared__ float tl[32][33];
  const int G4 = 4 * H;
  const int j0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) tl[r][tx] = whh[(long)(j0 + r) * H + k0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8) whhT[(long)(k0 + r) * G4 + j0 + tx] = tl[tx][r];
}

// backward step t.  Clip b at t >= L writes zero dgates (so the recurrent sum into its step L - 1
// vanishes on its own) and leaves its carry alone; at t = L - 1 it takes dhn / dcn as the fixed-length
// kernel does at T - 1.
__global__ __launch_bounds__(256) void lstm_bwd_step_vl_kernel(const float* __restrict__ dout, const float* __restrict__ dhn,
                                                               const float* __restrict__ dcn, const float* __restrict__ whhT,
                                                               const float* __restrict__ cst, const float* __restrict__ gates,
                                                               float* __restrict__ dgates, float* __restrict__ dcw,
                                                               const int* __restrict__ lens, int B, int T, int H, int t) {
  extern __shared__ float sm[];   // W columns [16 slices][SP] ([4H / 16][2] each), dh [B][2]
  const int G4 = 4 * H;
  const int per = G4 / 16, SP = 2 * per + 4;
  float* swc = sm;
  float* sdh = sm + 16 * SP;
  const int tid = threadIdx.x, u0 = blockIdx.x * LS_UPW;
  if (t < T - 1) {
    const int n4 = G4 / 4;
    const float4* r0 = reinterpret_cast<const float4*>(whhT + (long)u0 * G4);
    const float4* r1 = reinterpret_cast<const float4*>(whhT + (long)(u0 + 1) * G4);
    for (int e0 = tid; e0 < n4; e0 += 4 * 256) {
      float4 x0[4], x1[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = min(e0 + i * 256, n4 - 1);
        x0[i] = r0[e];
        x1[i] = r1[e];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = e0 + i * 256;
        if (e < n4) {   // jj = 4e..4e+3, all in slice 4e / per
          float4* d = reinterpret_cast<float4*>(swc + (4 * e / per) * SP + 2 * (4 * e % per));
          d[0] = make_float4(x0[i].x, x1[i].x, x0[i].y, x1[i].y);
          d[1] = make_float4(x0[i].z, x1[i].z, x0[i].w, x1[i].w);
        }
      }
    }
    __syncthreads();
    for (int b0 = 0; b0 < B; b0 += 16) {
      const int b = b0 + (tid >> 4), sl = tid & 15;
      float a0 = 0.f, a1 = 0.f;
      if (b < B) {
        const float* dg = dgates + ((long)b * T + t + 1) * G4 + sl * per;
        const float* wc = swc + sl * SP;
        for (int i0 = 0; i0 < per; i0 += 64) {
          float4 g4[16];
#pragma unroll
          for (int q = 0; q < 16; ++q) g4[q] = *reinterpret_cast<const float4*>(dg + i0 + 4 * q);
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const float gv[4] = {g4[q].x, g4[q].y, g4[q].z, g4[q].w};
            const float4* w4 = reinterpret_cast<const float4*>(wc + 2 * (i0 + 4 * q));
            const float4 wa = w4[0], wb = w4[1];
            const float wv[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              a0 = fmaf(gv[e], wv[2 * e], a0);
              a1 = fmaf(gv[e], wv[2 * e + 1], a1);
            }
          }
        }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        a0 += __shfl_xor(a0, o, 64);
        a1 += __shfl_xor(a1, o, 64);
      }
      if (sl == 0 && b < B) {
        sdh[b * 2] = a0;
        sdh[b * 2 + 1] = a1;
      }
    }
    __syncthreads();
  }
  if (tid < B * LS_UPW) {
    const int b = tid / LS_UPW, v = tid - b * LS_UPW, k = u0 + v;
    const int L = vl_len(lens, b, T);
    const bool live = t < L;
    const long ob = ((long)b * T + t) * H, bk = (long)b * H + k;
    // every global load unconditional (absent operands, and every operand of a clip past its end,
    // read a valid stand-in address and are selected away)
    const bool last = t == L - 1;
    const float* pc = cst + ob + k;
    const float vhn = *(last && dhn ? dhn + bk : pc);
    const float vcw = *(!last ? dcw + bk : (dcn ? dcn + bk : pc));
    const float vdo = *(dout ? dout + ob + k : pc);
    const float vcp = *(t > 0 ? pc - H : pc);
    const float c = *pc;
    const float* gt = gates + ((long)b * T + t) * G4;
    const float ig = gt[k], fg = gt[H + k], gg = gt[2 * H + k], og = gt[3 * H + k];
    // (t < T - 1 whenever !last && live, so sdh was written above)
    const float dhr = !last ? sdh[b * 2 + v] : (dhn ? vhn : 0.f);
    const float dcr = !last || dcn ? vcw : 0.f;
    const float dh = dhr + (dout ? vdo : 0.f);
    const float cp = t > 0 ? vcp : 0.f;
    const float tc = tanhf(c);
    const float dO = dh * tc;
    // dcr + dh * og * (1 - tc * tc), its roundings spelled out: in lstm_bwd_step_kernel hipcc pairs tc * tc
    // with dh * og into one packed multiply, so the product is rounded before the subtraction there (here
    // it would contract it into an fma); written this way the two kernels round alike
    const float dc = fmaf(dh * og, one_minus_sq_unfused(tc), dcr);
    const float dI = dc * gg, dG = dc * ig, dF = dc * cp;
    float* dg = dgates + ((long)b * T + t) * G4;
    if (live) {
      dcw[bk] = dc * fg;
      dg[k] = dI * ig * (1.f - ig);
      dg[H + k] = dF * fg * (1.f - fg);
      dg[2 * H + k] = dG * (1.f - gg * gg);
      dg[3 * H + k] = dO * og * (1.f - og);
    } else {
      dg[k] = 0.f;
      dg[H + k] = 0.f;
      dg[2 * H + k] = 0.f;
      dg[3 * H + k] = 0.f;
    }
  }
}

// Kernel choice: lstm.hip's rule without its persistent forms (the same predicates, restated here
// because that file's are local to it; `kernel`: 0 = automatic, 1 = the generic pair).
bool vl_reg(int H, int kernel) { return kernel == 0 && (H == 128 || H == 64); }
bool vl_step(int B, int H, int kernel) {
  const size_t fwd_lds = ((size_t)B * 32 * (H / 32 + 4) + 8 * B) * sizeof(float);
  const size_t bwd_lds = ((size_t)8 * H + 64 + 2 * B) * sizeof(float);
  return kernel == 0 && !vl_reg(H, kernel) && (H == 256 || H == 512 || H == 1024) && B <= LS_MAXB &&
         fwd_lds <= 65536 && bwd_lds <= 65536;
}

}  // namespace


extern "C" {

// 1 when xcp_lstm_fwd_varlen (same B, H, kernel) runs the generic kernel, which reads the transposed W_hh
int xcp_lstm_varlen_needs_whhT(int B, int H, int kernel) { return vl_reg(H, kernel) || vl_step(B, H, kernel) ? 0 : 1; }

int xcp_lstm_fwd_varlen(const float* xproj, const float* whh, const float* whhT, const float* bih, const float* bhh,
                        float* out, float* hprev, float* cst, float* gates, float* hn, float* cn, const int* lens, int B,
                        int T, int H, int kernel, hipStream_t st) {
  if (B <= 0 || T <= 0) return XCP_OK;
  if (kernel < 0 || kernel > 1 || H <= 0 || !lens) return XCP_EINVAL;
  if (vl_reg(H, kernel)) {
    if (H == 128)
      hipLaunchKernelGGL(lstm_fwd_reg_vl_kernel<128>, dim3(B), dim3(1024), 0, st, xproj, whh, bih, bhh, out, hprev, cst,
                         gates, hn, cn, lens, T);
    else
      hipLaunchKernelGGL(lstm_fwd_reg_vl_kernel<64>, dim3(B), dim3(1024), 0, st, xproj, whh, bih, bhh, out, hprev, cst,
                         gates, hn, cn, lens, T);
    return (int)hipGetLastError();
  }
  if (vl_step(B, H, kernel)) {
    const size_t smem = ((size_t)B * 32 * (H / 32 + 4) + 8 * B) * sizeof(float);
    for (int t = 0; t < T; ++t) {
      if (H == 256)
        hipLaunchKernelGGL(lstm_fwd_step_vl_kernel<8>, dim3(H / LS_UPW), dim3(256), smem, st, xproj, whh, bih, bhh, out,
                           hprev, cst, gates, hn, cn, lens, B, T, t);
      else if (H == 512)
        hipLaunchKernelGGL(lstm_fwd_step_vl_kernel<16>, dim3(H / LS_UPW), dim3(256), smem, st, xproj, whh, bih, bhh, out,
                           hprev, cst, gates, hn, cn, lens, B, T, t);
      else
        hipLaunchKernelGGL(lstm_fwd_step_vl_kernel<32>, dim3(H / LS_UPW), dim3(256), smem, st, xproj, whh, bih, bhh, out,
                           hprev, cst, gates, hn, cn, lens, B, T, t);
    }
    return (int)hipGetLastError();
  }
  if (!whhT) return XCP_EINVAL;
  const size_t smem = (size_t)6 * H * sizeof(float);
  hipLaunchKernelGGL(lstm_fwd_vl_kernel, dim3(B), dim3(256), smem, st, xproj, whhT, bih, bhh, out, hprev, cst, gates, hn,
                     cn, lens, T, H);
  return (int)hipGetLastError();
}

int xcp_lstm_bwd_varlen(const float* dout, const float* dhn, const float* dcn, const float* whh, const float* cst,
                        const float* gates, float* dgates, float* work, const int* lens, int B, int T, int H, int kernel,
                        hipStream_t st) {
  if (B <= 0 || T <= 0) return XCP_OK;
  if (kernel < 0 || kernel > 1 || H <= 0 || !lens) return XCP_EINVAL;
  if (vl_step(B, H, kernel)) {
    if (!work) return XCP_EINVAL;
    float* whhT = work + (long)B * H;
    hipLaunchKernelGGL(lstm_transpose_vl_kernel, dim3(4 * H / 32, H / 32), dim3(256), 0, st, whh, whhT, H);
    const size_t smem = ((size_t)8 * H + 64 + 2 * B) * sizeof(float);
    for (int t = T - 1; t >= 0; --t)
      hipLaunchKernelGGL(lstm_bwd_step_vl_kernel, dim3(H / LS_UPW), dim3(256), smem, st, dout, dhn, dcn, whhT, cst, gates,
                         dgates, work, lens, B, T, H, t);
    return (int)hipGetLastError();
  }
  if (vl_reg(H, kernel)) {
    if (H == 128)
      hipLaunchKernelGGL(lstm_bwd_reg_vl_kernel<128>, dim3(B), dim3(1024), 0, st, dout, dhn, dcn, whh, cst, gates, dgates,
                         lens, T);
    else
      hipLaunchKernelGGL(lstm_bwd_reg_vl_kernel<64>, dim3(B), dim3(1024), 0, st, dout, dhn, dcn, whh, cst, gates, dgates,
                         lens, T);
    return (int)hipGetLastError();
  }
  const size_t smem = (size_t)6 * H * sizeof(float);
  hipLaunchKernelGGL(lstm_bwd_vl_kernel, dim3(B), dim3(256), smem, st, dout, dhn, dcn, whh, cst, gates, dgates, lens, T, H);
  return (int)hipGetLastError();
}

}  // extern "C"
