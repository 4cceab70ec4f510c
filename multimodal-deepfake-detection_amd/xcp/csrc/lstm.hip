// Fused single-layer LSTM recurrence (batch_first, gate order i,f,g,o, h0=c0=0),
// forward and backward-through-time, fp32.
//
// Reference op: nn.LSTM(input_size=2048, hidden_size=H, num_layers=1,
// batch_first=True) (XceptionLSTMV.py:18-23, XceptionLSTMA.py:14-19), called at
// XceptionLSTMV.py:67 / XceptionLSTMA.py:56 and directly as
// `model.lstm(features)[0]` in train_visual.py:569.
//
// The input projection x W_ih^T for all T steps is one MFMA GEMM (gemm.hip);
// these kernels run the serial part: one workgroup per clip walks the T steps,
// keeping h in LDS and reading W_hh^T (coalesced across gate lanes) from L2.
//
// Per-clip lengths.  The generic, register-resident and per-step kernels are templates on
// `bool VL`: the VL = false instantiation is the fixed-length kernel (it never touches `lens`, its
// last argument), the VL = true one takes zero-padded clips of unequal length (lens [B], int,
// device memory; clamped here to [0, T]).  Both are one body, so with lens[b] = T the results are
// bit-identical to the fixed-length call (tests/test_gpu_lstm_varlen.py pins that per family); where
// the compiler could contract a cell expression differently per instantiation its roundings are
// spelled out.  The semantics are those of pack_padded_sequence -> nn.LSTM ->
// pad_packed_sequence(total_length = T): for clip b with L = lens[b], out[b][t] is h_t for t < L and
// zero for t >= L, h_n / c_n are the state after step L - 1 (zero for L = 0); the backward ignores
// dout[b][t >= L], takes dh_n / dc_n in at step L - 1 and writes zero pre-activation gradients for
// t >= L, so the clip adds nothing to any gradient from its padding and dx[b][t >= L] is exactly
// zero.
//   register-resident (H = 64 / 128) and generic: one workgroup per clip, L is workgroup-uniform;
//     the workgroup walks its clip's L steps, zero-fills its tail rows and leaves;
//   per-step (H = 256 / 512 / 1024, B <= 32): the (clip, unit) cell threads are masked per clip.
// A call with lengths never takes the persistent, gather or clip-grouped kernels below (H = 256 /
// 512 go to the per-step kernels): those hand steps over through polled counters with a timeout
// (the open findings in ADVICE.md), and nothing length-aware polls, counts or can time out.
//
// Saved state for t >= L: hprev is written (zero) because the weight gradient dW_hh = dgates^T hprev
// runs over all B*T rows and 0 x (uninitialised) may be NaN; cst and gates are left unwritten there
// and no kernel uses a value loaded from such a row (the per-step kernels load some as stand-in
// addresses and select them away, as they do for absent operands).
//
// Initial state.  The same three families are templates on `bool ST` as well: ST = false is the kernel
// above (h0 = c0 = 0; it never touches its state arguments, the last ones), ST = true starts clip b from
// h0[b] / c0[b] (fp32 [B][H]) -- nn.LSTM(...)(x, (h0, c0)), with lengths the same over packed input:
//   forward : h_{-1} = h0[b], c_{-1} = c0[b]; the saved hprev[b][0] is h0[b] (dW_hh = dgates^T hprev must
//     see it); h_n / c_n are the state after step L - 1 and, for L = 0, h0[b] / c0[b] themselves, so the
//     state passes through a clip that has no frame in this call (its out / hprev rows are zero as ever);
//   backward: step 0 takes c0 as c_{t-1}; after it dh0[b] = sum_j dgates_0[b][j] W_hh[j][:] and
//     dc0[b] = dc_0 f_0; for L = 0, dh0 = dh_n and dc0 = dc_n (zero where absent).  dh0 / dc0 may be null.
//     The per-clip kernels hold exactly these values in their carries when the loop ends; the per-step
//     backward forms dh_{t-1} in the next launch, so dh0 takes one more launch (t = -1) that runs the
//     recurrent sum alone and copies the cell-gradient carry out of `work`.
// One body again: hx = zeros is bit-identical to no state, and a sequence run in chunks with h_n / c_n
// carried into h0 / c0 (and dh0 / dc0 back into dh_n / dc_n) is bit-identical to the whole run in out,
// h_n, c_n, cst and dgates (tests/test_gpu_lstm_state.py).  A call with a state never takes the
// persistent, gather or clip-grouped kernels: nothing new polls.  h0 / c0 must not alias h_n / c_n.
//
// Directions.  The same three families are templates on `bool DR` as well: DR = false is the kernel above (it
// never touches its last argument, LstmDirs), DR = true is nn.LSTM(I, H, 1, batch_first=True,
// bidirectional=True): the grid's y index is a slot on the leading axis of every stacked array (whh
// [D][4H][H], bih / bhh [D][4H], xproj / gates / dgates [D][B*T][4H], hprev / cst [D][B][T][H], h0 / c0 / hn /
// cn / dh0 / dc0 [D][B][H]) and a column block of out / dout [B][T][D*H], which are written and read in place
// through a row pitch.  The reverse direction is the same cell on mirrored time inside the clip's own length:
//   per-clip families: step s of the walk works at time t = L - 1 - s, and "the row of step s - 1" is t + 1
//     instead of t - 1 -- nothing else differs, so the state enters at t = L - 1, hprev[L - 1] is h0, hn / cn
//     are the state after time 0 and dh0 / dc0 are the carries after the backward's last step, by the same code;
//   per-step family: launch s works at time s in the forward direction and T - 1 - s in the reverse one (the
//     direction is workgroup-uniform), so a pass stays T launches.  A reverse clip is dead FIRST in the forward
//     pass (t >= L: zero out / hprev) and starts at its own t = L - 1: where the forward direction's "t = 0"
//     is launch-uniform, "takes the state (or zero) as h_{prev}" is a per-clip select in the staging loop and
//     the cell.  Its backward walks time upwards: dhn / dcn enter at t = 0, the recurrent sum reads dgates of
//     row t - 1, c_{prev} is cst[t + 1] (c0 at L - 1), the clip goes dead at the END (zero dgates, carry
//     left alone), and the dh0 launch sums over each clip's own row L_b - 1.
// Direction 0 through the DR kernels is bit-identical to the kernels above, the reverse direction to the forward
// one on input mirrored inside each length (tests/test_gpu_lstm_bidir.py).  Never a kernel that polls.
#include "common.h"
#include <stdlib.h>
#include <mutex>
#include <utility>
#include <vector>

namespace {

XCP_DEV float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// 1 - v * v with the product rounded before the subtraction (no fma contraction)
XCP_DEV float one_minus_sq_unfused(float v) {
#pragma clang fp contract(off)
  const float p = v * v;
  return 1.f - p;
}

XCP_DEV int lstm_len(const int* __restrict__ lens, int b, int T) { return min(max(lens[b], 0), T); }

// Direction-aware call (template parameter DR of the generic, register-resident and per-step kernels; see
// "Directions" in the header comment).  The grid's y index is the slot on the stacked arrays' leading axis.
struct LstmDirs {
  int rev0;   // 1: slot 0 is the reverse direction (dirs = 2); slot 1 always is
  int op;     // row pitch of out / dout in floats (D * H); slot di starts at column di * H
};

// xproj [B][T][4H] (already x W_ih^T); whhT [H][4H]; bias = b_ih + b_hh added here.
// Outputs: out/h [B][T][H], hprev [B][T][H] (h_{t-1}), c [B][T][H],
// gates [B][T][4H] post-activation (i, f, g, o), h_n / c_n [B][H].
template <bool VL, bool ST, bool DR = false>
__global__ __launch_bounds__(256) void lstm_fwd_kernel(const float* __restrict__ xproj, const float* __restrict__ whhT,
                                                       const float* __restrict__ bih, const float* __restrict__ bhh,
                                                       float* __restrict__ out, float* __restrict__ hprev,
                                                       float* __restrict__ cst, float* __restrict__ gates,
                                                       float* __restrict__ hn, float* __restrict__ cn, int T, int H,
                                                       const int* __restrict__ lens, const float* __restrict__ h0,
                                                       const float* __restrict__ c0, LstmDirs dd) {
  extern __shared__ float sm[];   // h [H], c [H], gate pre-activations [4H]
  float* sh = sm;
  float* sc = sm + H;
  float* sg = sm + 2 * H;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int G4 = 4 * H;
  const int L = VL ? lstm_len(lens, b, T) : T;
  bool rev = false;   // workgroup-uniform
  int OP = H;
  if constexpr (DR) {
    const long di = blockIdx.y, nb = gridDim.x;
    rev = (dd.rev0 | (int)di) != 0;
    OP = dd.op;
    xproj += di * nb * T * G4; whhT += di * H * G4; bih += di * G4; bhh += di * G4;
    out += di * H; hprev += di * nb * T * H; cst += di * nb * T * H; gates += di * nb * T * G4;
    hn += di * nb * H; cn += di * nb * H;
    if constexpr (ST) { h0 += di * nb * H; c0 += di * nb * H; }
  }
  if constexpr (ST) {   // h_{-1}, c_{-1}: step 0 saves h0 as its hprev, and L = 0 hands both on as h_n / c_n
    for (int k = tid; k < H; k += blockDim.x) { sh[k] = h0[(long)b * H + k]; sc[k] = c0[(long)b * H + k]; }
  } else {
    for (int k = tid; k < H; k += blockDim.x) { sh[k] = 0.f; sc[k] = 0.f; }
  }
  __syncthreads();
  for (int s = 0; s < L; ++s) {
    const int t = DR && rev ? L - 1 - s : s;   // the reverse direction visits L - 1 .. 0
    const float* xp = xproj + ((long)b * T + t) * G4;
    for (int j = tid; j < G4; j += blockDim.x) {
      float acc = xp[j] + bih[j] + bhh[j];
      for (int k = 0; k < H; ++k) acc = fmaf(sh[k], whhT[(long)k * G4 + j], acc);
      sg[j] = acc;
    }
    __syncthreads();
    float* gt = gates + ((long)b * T + t) * G4;
    const long ob = ((long)b * T + t) * H;
    const long oo = DR ? ((long)b * T + t) * OP : ob;
    for (int k = tid; k < H; k += blockDim.x) {
      const float ig = sigm(sg[k]), fg = sigm(sg[H + k]), gg = tanhf(sg[2 * H + k]), og = sigm(sg[3 * H + k]);
      const float c = fmaf(fg, sc[k], ig * gg);
      const float h = og * tanhf(c);
      gt[k] = ig; gt[H + k] = fg; gt[2 * H + k] = gg; gt[3 * H + k] = og;
      hprev[ob + k] = sh[k];
      cst[ob + k] = c;
      out[oo + k] = h;
    }
    __syncthreads();
    for (int k = tid; k < H; k += blockDim.x) {
      sh[k] = out[oo + k];
      sc[k] = cst[ob + k];
    }
    __syncthreads();
  }
  for (int k = tid; k < H; k += blockDim.x) {
    hn[(long)b * H + k] = sh[k];
    cn[(long)b * H + k] = sc[k];
  }
  if constexpr (VL) {   // tail rows t >= L (contiguous): out and hprev zero (H is arbitrary here: 4-B stores)
    const long tb = ((long)b * T + L) * H, tn = (long)(T - L) * H;
    for (long e = tid; e < tn; e += blockDim.x) {
      if constexpr (DR) out[((long)b * T + L + e / H) * OP + e % H] = 0.f;
      else out[tb + e] = 0.f;
      hprev[tb + e] = 0.f;
    }
  }
}

// Backward through time.  dout [B][T][H] (may be null = zeros), dhn/dcn [B][H]
// (may be null).  whh [4H][H] (row-major, as stored by nn.LSTM).
// Writes dgates [B][T][4H] (pre-activation gradients).
template <bool VL, bool ST, bool DR = false>
__global__ __launch_bounds__(256) void lstm_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ dhn,
                                                       const float* __restrict__ dcn, const float* __restrict__ whh,
                                                       const float* __restrict__ cst, const float* __restrict__ gates,
                                                       float* __restrict__ dgates, int T, int H,
                                                       const int* __restrict__ lens, const float* __restrict__ c0,
                                                       float* __restrict__ dh0, float* __restrict__ dc0, LstmDirs dd) {
  extern __shared__ float sm[];   // dh [H], dc [H], dgates_t [4H]
  float* sdh = sm;
  float* sdc = sm + H;
  float* sdg = sm + 2 * H;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int G4 = 4 * H;
  const int L = VL ? lstm_len(lens, b, T) : T;
  bool rev = false;   // workgroup-uniform
  int OP = H;
  if constexpr (DR) {
    const long di = blockIdx.y, nb = gridDim.x;
    rev = (dd.rev0 | (int)di) != 0;
    OP = dd.op;
    if (dout) dout += di * H;
    if (dhn) dhn += di * nb * H;
    if (dcn) dcn += di * nb * H;
    whh += di * G4 * H; cst += di * nb * T * H; gates += di * nb * T * G4; dgates += di * nb * T * G4;
    if constexpr (ST) {
      if (c0) c0 += di * nb * H;
      if (dh0) dh0 += di * nb * H;
      if (dc0) dc0 += di * nb * H;
    }
  }
  for (int k = tid; k < H; k += blockDim.x) {
    sdh[k] = dhn ? dhn[(long)b * H + k] : 0.f;
    sdc[k] = dcn ? dcn[(long)b * H + k] : 0.f;
  }
  __syncthreads();
  for (int s = L - 1; s >= 0; --s) {   // s: the forward pass's step; time t is mirrored for the reverse direction
    const int t = DR && rev ? L - 1 - s : s;
    const long ob = ((long)b * T + t) * H;
    const long oo = DR ? ((long)b * T + t) * OP : ob;
    const float* gt = gates + ((long)b * T + t) * G4;
    float* dg = dgates + ((long)b * T + t) * G4;
    for (int k = tid; k < H; k += blockDim.x) {
      const float dh = sdh[k] + (dout ? dout[oo + k] : 0.f);
      const float c = cst[ob + k];
      float cp = 0.f;   // c of step s - 1: the row before, or for the reverse direction the row after
      if constexpr (ST) cp = s > 0 ? cst[(DR && rev ? ob + H : ob - H) + k] : (c0 ? c0[(long)b * H + k] : 0.f);
      else cp = s > 0 ? cst[(DR && rev ? ob + H : ob - H) + k] : 0.f;
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
  if constexpr (ST) {   // what is left after step 0 (for L = 0: dh_n / dc_n, or zero) is the state's gradient
    for (int k = tid; k < H; k += blockDim.x) {
      if (dh0) dh0[(long)b * H + k] = sdh[k];
      if (dc0) dc0[(long)b * H + k] = sdc[k];
    }
  }
  if constexpr (VL) {   // tail rows t >= L: zero pre-activation gradients
    const long tb = ((long)b * T + L) * G4, tn = (long)(T - L) * G4;
    for (long e = tid; e < tn; e += blockDim.x) dgates[tb + e] = 0.f;
  }
}


// ---------------------------------------------------------------------------------
// Register-resident recurrence for H <= 128 (XceptionLSTMV: H = 128).  One 1024-thread
// workgroup per clip holds the whole W_hh in VGPRs (4H*H/1024 = 64 fp32 per thread at
// H = 128), so a time step is KPT FMAs per thread against h broadcast from LDS, an
// S-lane shuffle reduction and the cell math: no global traffic on the serial path
// except the per-step x-projection / state rows, which are prefetched one step ahead.
//
// forward: thread (gate j, part s), tid = j*S + s, holds W_hh[j][s*KPT .. +KPT).
template <int H, bool VL, bool ST, bool DR = false>
__global__ __launch_bounds__(1024) void lstm_fwd_reg_kernel(const float* __restrict__ xproj,
                                                            const float* __restrict__ whh,
                                                            const float* __restrict__ bih,
                                                            const float* __restrict__ bhh, float* __restrict__ out,
                                                            float* __restrict__ hprev, float* __restrict__ cst,
                                                            float* __restrict__ gates, float* __restrict__ hn,
                                                            float* __restrict__ cn, int T,
                                                            const int* __restrict__ lens,
                                                            const float* __restrict__ h0,
                                                            const float* __restrict__ c0, LstmDirs dd) {
  constexpr int G4 = 4 * H, S = 1024 / G4, KPT = H / S, PADK = KPT + 4;
  static_assert(S >= 1 && KPT % 4 == 0, "unsupported H");
  __shared__ __attribute__((aligned(16))) float sh[S * PADK];   // h_{t-1}, part s at s*PADK (bank-spread)
  __shared__ float sg[G4];                                      // activated gates of step t
  const int tid = threadIdx.x, b = blockIdx.x;
  const int L = VL ? lstm_len(lens, b, T) : T;   // workgroup-uniform
  bool rev = false;                              // workgroup-uniform
  int OP = H;
  if constexpr (DR) {
    const long di = blockIdx.y, nb = gridDim.x;
    rev = (dd.rev0 | (int)di) != 0;
    OP = dd.op;
    xproj += di * nb * T * G4; whh += di * G4 * H; bih += di * G4; bhh += di * G4;
    out += di * H; hprev += di * nb * T * H; cst += di * nb * T * H; gates += di * nb * T * G4;
    hn += di * nb * H; cn += di * nb * H;
    if constexpr (ST) { h0 += di * nb * H; c0 += di * nb * H; }
  }
  // time of step q: the reverse direction visits L - 1 .. 0
  auto tof = [&](int q) { return DR && rev ? L - 1 - q : q; };
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
  float c = 0.f;                                 // c_{t-1}[tid] for tid < H
  if constexpr (ST) {   // h_{-1}, c_{-1} (for L = 0 they are handed on as h_n / c_n below)
    if (tid < H) {
      sh[hidx(tid)] = h0[(long)b * H + tid];
      c = c0[(long)b * H + tid];
    }
  } else {
    if (tid < H) sh[hidx(tid)] = 0.f;
  }
  const float* xb = xproj + (long)b * T * G4;
  float xn = s == 0 ? xb[(long)(DR ? max(tof(0), 0) : 0) * G4 + j] : 0.f;   // (row 0 exists for L = 0 too: T >= 1)
  __syncthreads();
  for (int q = 0; q < L; ++q) {
    const int t = tof(q);
    const float xc = xn;
    if (s == 0 && q + 1 < L) xn = xb[(long)tof(q + 1) * G4 + j];
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
      out[DR ? ((long)b * T + t) * OP + tid : ob] = h;
      sh[hidx(tid)] = h;      // every read of h_{t-1} happened before the barrier above
    }
    __syncthreads();
  }
  if (tid < H) {
    hn[(long)b * H + tid] = sh[hidx(tid)];
    cn[(long)b * H + tid] = c;
  }
  if constexpr (VL) {
    // tail rows t >= L, contiguous from row b*T + L (a multiple of H floats: 16-B aligned): out and
    // hprev zero, one float4 per thread and pass
    const long n4 = (long)(T - L) * (H / 4);
    float4* po = reinterpret_cast<float4*>(out + ((long)b * T + L) * H);
    float4* ph = reinterpret_cast<float4*>(hprev + ((long)b * T + L) * H);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long e = tid; e < n4; e += 1024) {
      if constexpr (DR) *reinterpret_cast<float4*>(out + ((long)b * T + L + e / (H / 4)) * OP + e % (H / 4) * 4) = z;
      else po[e] = z;
      ph[e] = z;
    }
  }
}

// backward: thread (unit k, part p), tid = k*P + p, holds W_hh[p*JPT .. +JPT)[k]; the
// step's pre-activation gradients are broadcast from LDS and dh_{t-1}[k] is reduced over
// the P parts (adjacent lanes) by shuffles.
template <int H, bool VL, bool ST, bool DR = false>
__global__ __launch_bounds__(1024) void lstm_bwd_reg_kernel(const float* __restrict__ dout,
                                                            const float* __restrict__ dhn,
                                                            const float* __restrict__ dcn,
                                                            const float* __restrict__ whh,
                                                            const float* __restrict__ cst,
                                                            const float* __restrict__ gates,
                                                            float* __restrict__ dgates, int T,
                                                            const int* __restrict__ lens,
                                                            const float* __restrict__ c0,
                                                            float* __restrict__ dh0, float* __restrict__ dc0,
                                                            LstmDirs dd) {
  constexpr int G4 = 4 * H, P = 1024 / H, JPT = G4 / P, PADJ = JPT + 4;
  static_assert(P >= 1 && JPT % 4 == 0, "unsupported H");
  __shared__ __attribute__((aligned(16))) float sdg[P * PADJ];
  __shared__ float sdh[H];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int L = VL ? lstm_len(lens, b, T) : T;   // workgroup-uniform
  bool rev = false;                              // workgroup-uniform
  int OP = H;
  if constexpr (DR) {
    const long di = blockIdx.y, nb = gridDim.x;
    rev = (dd.rev0 | (int)di) != 0;
    OP = dd.op;
    if (dout) dout += di * H;
    if (dhn) dhn += di * nb * H;
    if (dcn) dcn += di * nb * H;
    whh += di * G4 * H; cst += di * nb * T * H; gates += di * nb * T * G4; dgates += di * nb * T * G4;
    if constexpr (ST) {
      if (c0) c0 += di * nb * H;
      if (dh0) dh0 += di * nb * H;
      if (dc0) dc0 += di * nb * H;
    }
  }
  const int k = tid / P, p = tid % P;
  float w[JPT];
#pragma unroll
  for (int q = 0; q < JPT; ++q) w[q] = whh[(long)(p * JPT + q) * H + k];
  auto gidx = [](int jj) { return (jj / JPT) * PADJ + jj % JPT; };
  float dc = 0.f;                                // dc carried into step t, unit tid < H
  // per-step inputs of unit tid, prefetched one step ahead
  float n_c = 0.f, n_cp = 0.f, n_i = 0.f, n_f = 0.f, n_g = 0.f, n_o = 0.f, n_do = 0.f;
  auto fetch = [&](int q) {   // q: the forward pass's step; its time is mirrored for the reverse direction
    const int t = DR && rev ? L - 1 - q : q;
    const long ob = ((long)b * T + t) * H + tid;
    const float* gt = gates + ((long)b * T + t) * G4;
    n_c = cst[ob];   // (c of step q - 1: the row before, or for the reverse direction the row after)
    if constexpr (ST) n_cp = q > 0 ? cst[DR && rev ? ob + H : ob - H] : (c0 ? c0[(long)b * H + tid] : 0.f);
    else n_cp = q > 0 ? cst[DR && rev ? ob + H : ob - H] : 0.f;
    n_i = gt[tid]; n_f = gt[H + tid]; n_g = gt[2 * H + tid]; n_o = gt[3 * H + tid];
    n_do = dout ? dout[DR ? ((long)b * T + t) * OP + tid : ob] : 0.f;
  };
  if (tid < H) {
    sdh[tid] = dhn ? dhn[(long)b * H + tid] : 0.f;
    dc = dcn ? dcn[(long)b * H + tid] : 0.f;
    if (!VL || L > 0) fetch(L - 1);
  }
  __syncthreads();
  for (int q = L - 1; q >= 0; --q) {
    const int t = DR && rev ? L - 1 - q : q;
    if (tid < H) {
      const float c = n_c, cp = n_cp, ig = n_i, fg = n_f, gg = n_g, og = n_o;
      const float dh = sdh[tid] + n_do;
      if (q > 0) fetch(q - 1);
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
  if constexpr (ST) {   // what is left after step 0 (for L = 0: dh_n / dc_n, or zero) is the state's gradient
    if (tid < H) {
      if (dh0) dh0[(long)b * H + tid] = sdh[tid];
      if (dc0) dc0[(long)b * H + tid] = dc;
    }
  }
  if constexpr (VL) {   // tail rows t >= L (contiguous, 16-B aligned): zero pre-activation gradients
    const long n4 = (long)(T - L) * (G4 / 4);
    float4* pd = reinterpret_cast<float4*>(dgates + ((long)b * T + L) * G4);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long e = tid; e < n4; e += 1024) pd[e] = z;
  }
}


// ---------------------------------------------------------------------------------
// Per-step kernels for large H (XceptionLSTMA: H = 512, T = 120).  One workgroup per clip
// cannot keep up there: it streams the whole W_hh (4H x H fp32 = 4 MB) through one CU per
// step (~530 us a step).  Here every time step is one launch spread over H / 2 workgroups
// (256 at H = 512), each owning 2 hidden units -- their 8 gate rows of W_hh (forward) or
// their 2 columns (backward); the launch boundary is the grid-wide step barrier and makes
// h_t / dgates_t visible to every CU.
//
// forward step t: thread (row r = gate q of unit uu, k-slice s of H/32) dots its W_hh row
// slice with h_{t-1} (staged in LDS, rows padded against bank conflicts) for every clip,
// the 32 slices reduce by shuffles, and (clip, unit) threads run the cell.
//
// With lengths every dot product still runs for every clip (a finished clip's h_{t-1} /
// dgates_{t+1} row is the zero this pair wrote, or the clip's last real row at t = L: finite either
// way, and nothing of that clip is read again); only the (clip, unit) cell threads look at the
// clip's length.
constexpr int LS_UPW = 2;              // hidden units per workgroup
constexpr int LS_MAXB = 32;            // clips (register partials per thread)

template <int KS, bool VL, bool ST, bool DR = false>   // KS = H / 32 (k values per slice)
__global__ __launch_bounds__(256) void lstm_fwd_step_kernel(const float* __restrict__ xproj, const float* __restrict__ whh,
                                                            const float* __restrict__ bih, const float* __restrict__ bhh,
                                                            float* __restrict__ out, float* __restrict__ hprev,
                                                            float* __restrict__ cst, float* __restrict__ gates,
                                                            float* __restrict__ hn, float* __restrict__ cn, int B, int T,
                                                            int t, const int* __restrict__ lens,
                                                            const float* __restrict__ h0, const float* __restrict__ c0,
                                                            LstmDirs dd) {
  constexpr int H = KS * 32, G4 = 4 * H, PS = KS + 4;   // LDS slice pitch (floats)
  constexpr int RP = 33;                                // pitch of a (row, clip) partial row
  extern __shared__ float sm[];   // h_{t-1} [B][32][PS] (then the partials [8][B][RP]), then pre [8][B]
  float* sh = sm;
  float* spre = sm + B * 32 * PS;
  const int tid = threadIdx.x, u0 = blockIdx.x * LS_UPW;
  // DR: launch s (the argument t) is time s for the forward direction and time T - 1 - s for the reverse
  // one, whose "previous" row is t + 1; a clip of the reverse direction starts (takes the state, or zero) at
  // its own t = L - 1, a per-clip condition where the forward direction's t = 0 is launch-uniform
  bool rev = false;   // workgroup-uniform
  int OP = H;
  if constexpr (DR) {
    const long di = blockIdx.y;
    rev = (dd.rev0 | (int)di) != 0;
    OP = dd.op;
    if (rev) t = T - 1 - t;
    xproj += di * B * T * G4; whh += di * G4 * H; bih += di * G4; bhh += di * G4;
    out += di * H; hprev += di * B * T * H; cst += di * B * T * H; gates += di * B * T * G4;
    hn += di * B * H; cn += di * B * H;
    if constexpr (ST) { h0 += di * B * H; c0 += di * B * H; }
  }
  const int r = tid >> 5, s = tid & 31, q = r >> 1, uu = r & 1;
  const int j = q * H + u0 + uu;
  // W_hh row slice
  float w[KS];
#pragma unroll
  for (int i = 0; i < KS; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(whh + (long)j * H + s * KS + i);
    w[i] = v.x; w[i + 1] = v.y; w[i + 2] = v.z; w[i + 3] = v.w;
  }
  // stage h_{t-1} (zero at t = 0): 8 loads in flight per thread -- unconditional (clamped index;
  // t = 0 reads step 0's slot as a stand-in and selects zero), since a load under a condition is
  // issued and waited for on its own.  With a state (ST) the t = 0 launch stages h0 [B][H] instead.
  const int n4 = B * H / 4;
  const int tp = t > 0 ? t - 1 : 0;
  for (int e0 = tid; e0 < n4; e0 += 8 * 256) {
    float4 v[8];
    [[maybe_unused]] bool fst[8];   // DR: the clip starts at this step (its h_{t-1} is the state, or zero)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = min(e0 + i * 256, n4 - 1);
      const int b = e / (H / 4), k4 = (e - b * (H / 4)) * 4;
      if constexpr (DR) {
        // reverse: row t + 1 (clamped), and the state at t >= L_b - 1 (a clip past its end stages the state or
        // zero: finite, and nothing of it is used)
        fst[i] = rev ? t + 1 >= (VL ? lstm_len(lens, b, T) : T) : t == 0;
        const int rp = rev ? min(t + 1, T - 1) : tp;
        const float* src = out + ((long)b * T + rp) * OP + k4;
        if constexpr (ST) src = fst[i] ? h0 + (long)b * H + k4 : src;
        v[i] = *reinterpret_cast<const float4*>(src);
      } else {
        const float* src = out + ((long)b * T + tp) * H + k4;
        if constexpr (ST) src = t > 0 ? src : h0 + (long)b * H + k4;
        v[i] = *reinterpret_cast<const float4*>(src);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = e0 + i * 256;
      const int b = e / (H / 4), k4 = (e - b * (H / 4)) * 4;
      bool keep = ST || t > 0;
      if constexpr (DR) keep = ST || !fst[i];
      if (e < n4)
        *reinterpret_cast<float4*>(sh + (b * 32 + k4 / KS) * PS + (k4 % KS)) =
            keep ? v[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __syncthreads();
  // every clip's partial dot of this thread's row slice, independent chains (no per-clip
  // cross-lane reduction on the critical path)
  float acc[LS_MAXB];
#pragma unroll
  for (int b = 0; b < LS_MAXB; ++b) {
    acc[b] = 0.f;
    if (b < B) {
      // 16-B reads (ds_read_b128, banks (a/4) % 64): the slices' pitch PS = KS + 4 puts every
      // lane group's 16 slices on distinct 4-bank slots (as 2-dword reads, banks mod 32, the same
      // pitch was a 4-way conflict: 71 % of this kernel's LDS cycles)
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
  // (row, clip) threads sum the 32 slices in the pairwise order of a 5-level xor butterfly
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
    const int L = VL ? lstm_len(lens, b, T) : T;
    const bool live = !VL || t < L;   // past the clip's end: zero out / hprev, no state, no saved gates
    const float* xp = xproj + ((long)b * T + t) * G4;
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int jj = g * H + k;
      pre[g] = spre[(g * 2 + v) * B + b] + xp[jj] + bih[jj] + bhh[jj];
    }
    const float ig = sigm(pre[0]), fg = sigm(pre[1]), gg = tanhf(pre[2]), og = sigm(pre[3]);
    const long ob = ((long)b * T + t) * H;
    const long oo = DR ? ((long)b * T + t) * OP : ob;
    const long op = t > 0 ? ob - H + k : ob + k;   // t = 0: a valid stand-in, selected away
    // (t > L: row t - 1 of cst was never written -- a valid address whose value is selected away)
    const float* pcp = cst + op;
    const float* php = out + op;
    // the clip has a previous step; reverse direction: not at t = L - 1, nor at any t past the end
    bool hasp = t > 0;
    if constexpr (DR) {
      if (rev) hasp = t + 1 < L;
      const long dp = !hasp ? 0 : (rev ? 1 : -1);   // no previous step: its own row, a valid stand-in, selected away
      pcp = cst + ob + dp * H + k;
      php = out + oo + dp * OP + k;
    }
    if constexpr (ST) {   // no previous step: the state itself
      pcp = hasp ? pcp : c0 + (long)b * H + k;
      php = hasp ? php : h0 + (long)b * H + k;
    }
    const float vcp = *pcp, vhp = *php;
    const float cp = ST || hasp ? vcp : 0.f;
    const float c = fmaf(fg, cp, ig * gg);
    const float h = og * tanhf(c);
    float* gt = gates + ((long)b * T + t) * G4;
    if (live) { gt[k] = ig; gt[H + k] = fg; gt[2 * H + k] = gg; gt[3 * H + k] = og; }
    hprev[ob + k] = live && (ST || hasp) ? vhp : 0.f;
    if (live) cst[ob + k] = c;
    out[oo + k] = live ? h : 0.f;
    if (DR && rev ? t == 0 && L > 0 : t == L - 1) {   // the clip's last step
      hn[(long)b * H + k] = h;
      cn[(long)b * H + k] = c;
    }
    if (VL && t == 0 && L == 0) {   // no frame: zero state, or the given one handed on
      hn[(long)b * H + k] = ST ? vhp : 0.f;
      cn[(long)b * H + k] = ST ? vcp : 0.f;
    }
  }
}

// whhT[k][j] = whh[j][k] (once per backward call, so a workgroup's W_hh columns are rows)
__global__ __launch_bounds__(256) void lstm_transpose_kernel(const float* __restrict__ whh, float* __restrict__ whhT,
                                                             int H) {
  __shared__ float tl[32][33];
  const int G4 = 4 * H;
  const int j0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) tl[r][tx] = whh[(long)(j0 + r) * H + k0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8) whhT[(long)(k0 + r) * G4 + j0 + tx] = tl[tx][r];
}

// backward step t: dh_t[b][k] = dout[b][t][k] + sum_j dgates_{t+1}[b][j] W_hh[j][k] (dhn at
// t = T-1): thread (clip b, j-slice sl of 4H/16) against the workgroup's 2 W_hh columns in
// LDS, 16-slice shuffle reduction; (clip, unit) threads run the cell backward with the cell
// gradient carried in dcw [B][H] (each unit's carry is only touched by its workgroup).
// With lengths, clip b at t >= L writes zero dgates (so the recurrent sum into its step L - 1
// vanishes on its own) and leaves its carry alone; at t = L - 1 it takes dhn / dcn as a full clip
// does at T - 1.
// DR: launch t (T - 1 .. 0, then -1 for dh0) is time t for the forward direction and time T - 1 - t for the
// reverse one, which therefore walks 0 .. T - 1: its recurrent sum reads dgates of row time - 1, it takes
// dhn / dcn at time 0, its c_{prev} is cst[time + 1] (c0 at L - 1), its clips go dead at the END of the walk
// (time >= L: zero dgates, carry left alone), and the dh0 launch sums over row L_b - 1 of each clip.
template <bool VL, bool ST, bool DR = false>
__global__ __launch_bounds__(256) void lstm_bwd_step_kernel(const float* __restrict__ dout, const float* __restrict__ dhn,
                                                            const float* __restrict__ dcn, const float* __restrict__ whhT,
                                                            const float* __restrict__ cst, const float* __restrict__ gates,
                                                            float* __restrict__ dgates, float* __restrict__ dcw, int B,
                                                            int T, int H, int t, const int* __restrict__ lens,
                                                            const float* __restrict__ c0, float* __restrict__ dh0,
                                                            float* __restrict__ dc0, LstmDirs dd) {
  extern __shared__ float sm[];   // W columns [16 slices][SP] ([4H / 16][2] each), dh [B][2]
  const int G4 = 4 * H;
  const int per = G4 / 16, SP = 2 * per + 4;   // slice pitch: +4 floats, so the 16 slices of a
                                               // half-wave start on 16 different 4-bank groups
  float* swc = sm;
  float* sdh = sm + 16 * SP;
  const int tid = threadIdx.x, u0 = blockIdx.x * LS_UPW;
  bool rev = false;   // workgroup-uniform
  int OP = H;
  if constexpr (DR) {
    const long di = blockIdx.y;
    rev = (dd.rev0 | (int)di) != 0;
    OP = dd.op;
    if (dout) dout += di * H;
    if (dhn) dhn += di * B * H;
    if (dcn) dcn += di * B * H;
    whhT += di * ((long)B * H + (long)G4 * H); dcw += di * ((long)B * H + (long)G4 * H);   // work: [D][carry, W_hh^T]
    cst += di * B * T * H; gates += di * B * T * G4; dgates += di * B * T * G4;
    if constexpr (ST) {
      if (c0) c0 += di * B * H;
      if (dh0) dh0 += di * B * H;
      if (dc0) dc0 += di * B * H;
    }
  }
  if (t < T - 1) {   // (the launch index: every launch but the first has a recurrent sum, in either direction)
    // rows u0, u0+1 of W_hh^T (contiguous), interleaved into swc[j][2]: 16-B loads, up to 4 per
    // row per thread issued before any store (clamped indices; a loop of dependent scalar loads
    // was ~8 L2 round trips a step at H = 512)
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
        const float* dg = dgates + ((long)b * T + t + 1) * G4 + sl * per;   // the row the previous launch wrote
        if constexpr (DR) {
          if (rev) {
            int rr = T - 2 - t;
            if constexpr (VL && ST)   // reverse dh0 launch: each clip's last live step is its own L_b - 1
              if (t < 0) rr = max(lstm_len(lens, b, T) - 1, 0);
            dg = dgates + ((long)b * T + rr) * G4 + sl * per;
          }
        }
        const float* wc = swc + sl * SP;
        // 16 independent 16-B loads in flight per batch (the loop is L2-latency-bound otherwise)
        for (int i0 = 0; i0 < per; i0 += 64) {
          float4 g4[16];
#pragma unroll
          for (int q = 0; q < 16; ++q) g4[q] = *reinterpret_cast<const float4*>(dg + i0 + 4 * q);
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const float gv[4] = {g4[q].x, g4[q].y, g4[q].z, g4[q].w};
            // (W[i][0], W[i][1], W[i+1][0], W[i+1][1]) as one ds_read_b128: banks (a/4) % 64, the
            // 16 slices 4 banks apart (pitch SP), so a lane group's reads never collide
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
    const int L = VL ? lstm_len(lens, b, T) : T;
    if constexpr (ST) {
      if (t < 0) {   // the launch after step 0: only the recurrent sum above ran (over dgates_0)
        const long bk = (long)b * H + k;
        const bool none = VL && L == 0;   // no frame: dh_n / dc_n (or zero) pass through; the carry was never written
        if (dh0) dh0[bk] = none ? (dhn ? dhn[bk] : 0.f) : sdh[b * 2 + v];
        if (dc0) dc0[bk] = none ? (dcn ? dcn[bk] : 0.f) : dcw[bk];
        return;
      }
    }
    if constexpr (DR) {
      if (rev) t = T - 1 - t;   // the time this launch works at
    }
    const bool live = !VL || t < L;
    const long ob = ((long)b * T + t) * H, bk = (long)b * H + k;
    // every global load unconditional (absent operands, and every operand of a clip past its end,
    // read a valid stand-in address and are selected away), so they go out together instead of one
    // round trip per branch
    bool last = t == L - 1;   // the step the backward enters at: takes dhn / dcn
    if constexpr (DR) {
      if (rev) last = t == 0;
    }
    const float* pc = cst + ob + k;
    const float vhn = *(last && dhn ? dhn + bk : pc);
    const float vcw = *(!last ? dcw + bk : (dcn ? dcn + bk : pc));
    const float* pdo = dout + ob + k;
    if constexpr (DR) pdo = dout + ((long)b * T + t) * OP + k;
    const float vdo = *(dout ? pdo : pc);
    bool hasp = t > 0;        // the forward pass had a step before this one
    const float* pcp = hasp ? pc - H : pc;
    if constexpr (DR) {
      if (rev) {
        hasp = t + 1 < L;
        pcp = hasp ? pc + H : pc;
      }
    }
    if constexpr (ST) pcp = hasp || !c0 ? pcp : c0 + bk;
    const float vcp = *pcp;
    const float c = *pc;
    const float* gt = gates + ((long)b * T + t) * G4;
    const float ig = gt[k], fg = gt[H + k], gg = gt[2 * H + k], og = gt[3 * H + k];
    // (not the first launch whenever !last && live, so sdh was written above)
    const float dhr = !last ? sdh[b * 2 + v] : (dhn ? vhn : 0.f);
    const float dcr = !last || dcn ? vcw : 0.f;
    const float dh = dhr + (dout ? vdo : 0.f);
    const float cp = hasp || (ST && c0) ? vcp : 0.f;
    const float tc = tanhf(c);
    const float dO = dh * tc;
    // dcr + dh * og * (1 - tc * tc) with its roundings spelled out: left to the compiler, one
    // instantiation pairs tc * tc with dh * og into a packed multiply (the product rounded before the
    // subtraction) and the other contracts it into an fma, and full lengths would no longer be
    // bit-identical to the call without lengths.  This is the rounding the fixed-length kernel has
    // always had.
    const float dc = fmaf(dh * og, one_minus_sq_unfused(tc), dcr);
    const float dI = dc * gg, dG = dc * ig, dF = dc * cp;
    if (live) dcw[bk] = dc * fg;
    float* dg = dgates + ((long)b * T + t) * G4;
    dg[k] = live ? dI * ig * (1.f - ig) : 0.f;
    dg[H + k] = live ? dF * fg * (1.f - fg) : 0.f;
    dg[2 * H + k] = live ? dG * (1.f - gg * gg) : 0.f;
    dg[3 * H + k] = live ? dO * og * (1.f - og) : 0.f;
  }
}

// ---------------------------------------------------------------------------------
// Persistent recurrence for H = 256 / 512 (XceptionLSTMA: H = 512, T = 120): ONE launch per
// direction walks all T steps, instead of the T launches of the per-step kernels above (each of
// which re-read its W_hh slice from L2 and paid a kernel boundary per step).
//
// G = H / 4 workgroups of 256 threads, each owning 4 hidden units for the whole launch, with
// their W_hh slice in VGPRs (one wave per SIMD, 128 fp32 weights per lane):
//   forward : lane l holds W_hh[16 gate rows of its units][k = l*KL .. +KL)  (KL = H / 64)
//   backward: lane l holds W_hh[j = l*JL .. +JL)[its 4 units]              (JL = 4H / 64)
// Wave v handles clips 16p + 4v .. +3 (pass p = 0, 1 for B <= 32).  A step's dot products are
// per-lane FMA chains over the lane's k (j) range; the 64 lanes' partial sums (16 rows x 4 clips
// forward, 4 units x 4 clips backward) are combined by a reduce-scatter butterfly (each xor level
// halves what a lane keeps), so after 6 levels lane l holds one complete (clip, row) sum
// (forward: clip l >> 4, row l & 15 = gate * 4 + unit; backward: clip l >> 4, unit (l >> 2) & 3).
// The cell runs on 16 lanes per wave with c (forward) / the cell-gradient carry (backward) kept
// in a register across steps.
// Step hand-off (guide: MI355X_MICROARCH.md "Valid forms", first table row): every store of
// h_t (forward) / dgates_t (backward) is a 4-B sc1 store; each storing wave waits vmcnt(0),
// the workgroup barriers, and one lane adds 1 to its shard counter (blockIdx % 8, one 128-B line
// each, agent-scope atomic).  Before a step, wave 0 polls the 8 shards with sc1 loads until each
// counted every one of its workgroups for the previous step, the workgroup barriers, and every
// load of the handed-off values is a 16-B sc1 buffer load.  Counters are zeroed by the host per
// launch; a poll that runs past ~LP_SPIN sleeps sets the error word and the workgroup leaves
// (the results are then invalid, but no wave spins forever: e.g. if fewer than G workgroups
// could ever be resident, which the host rules out with the occupancy query).
constexpr int LP_U = 4;                   // hidden units per workgroup
constexpr int LP_SHARD = 32;              // uints per shard counter (one 128-B line)
constexpr unsigned LP_SPIN = 1u << 22;    // polls (each after s_sleep 2) before giving up
constexpr int LP_CSP = 0x00020000;        // raw buffer descriptor word 3
constexpr int LP_SC1 = 16;                // cache policy: sc1

typedef int i32x4v __attribute__((ext_vector_type(4)));

struct LstmSync {
  unsigned* cnt;   // [8][LP_SHARD]
  unsigned* err;   // set to 1 on a poll timeout
};

// wave 0 waits until every shard has `steps` arrivals from each of its workgroups; then the
// workgroup barrier.  false (every thread) on a timeout.
XCP_DEV bool lp_wait(const LstmSync& sy, unsigned steps) {
  __shared__ int s_ok;
  const int tid = threadIdx.x, lane = tid & 63, G = gridDim.x;
  if (tid < 64) {
    const unsigned want = steps * (unsigned)(G / 8 + ((lane & 7) < G % 8 ? 1 : 0));
    unsigned it = 0;
    bool ok = false;
    while (true) {
      const unsigned v = lane < 8 ? __hip_atomic_load(sy.cnt + lane * LP_SHARD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                  : want;
      ok = __all(v >= want);
      if (ok || ++it > LP_SPIN) break;
      __builtin_amdgcn_s_sleep(2);
    }
    if (tid == 0) {
      s_ok = ok;
      if (!ok) __hip_atomic_store(sy.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  return s_ok != 0;
}

// every wave's sc1 stores have completed; then one arrival on this workgroup's shard
XCP_DEV void lp_publish(const LstmSync& sy) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_fetch_add(sy.cnt + (blockIdx.x % 8) * LP_SHARD, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

XCP_DEV void lp_st(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int V> struct LpIC {
  static constexpr int value = V;
};
template <int B, int E, typename F>
XCP_DEV void lp_static_for(F&& f) {
  if constexpr (B < E) {
    f(LpIC<B>{});
    lp_static_for<B + 1, E>(f);
  }
}

// reduce-scatter of v[N] over the 64 lanes: level d keeps the upper half where lane & d; after
// log2(N) levels lane l holds index (l >> (6 - log2 N)) complete over those lanes, the remaining
// levels sum plainly (every lane of a group ends with the same value).  Every index is a
// compile-time constant (the array stays in VGPRs).
template <int N>
XCP_DEV float lp_rscatter(float (&v)[N], int lane) {
  lp_static_for<0, 6>([&](auto L) {
    constexpr int d = 32 >> decltype(L)::value;
    constexpr int n = N >> decltype(L)::value;
    if constexpr (n >= 2) {
      const bool up = lane & d;
#pragma unroll
      for (int c = 0; c < n / 2; ++c) {
        const float keep = up ? v[n / 2 + c] : v[c];
        const float send = up ? v[c] : v[n / 2 + c];
        v[c] = keep + __shfl_xor(send, d, 64);
      }
    } else {
      v[0] += __shfl_xor(v[0], d, 64);
    }
  });
  return v[0];
}

// (one wave per SIMD: the whole 512-entry register file, so a step's loads all go out before the
// first use -- at 256 registers hipcc issued them clip by clip, one L2 round trip each)
template <int H>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void lstm_fwd_persist_kernel(const float* __restrict__ xproj, const float* __restrict__ whh,
                             const float* __restrict__ bih, const float* __restrict__ bhh, float* out,
                             float* __restrict__ hprev, float* __restrict__ cst, float* __restrict__ gates,
                             float* __restrict__ hn, float* __restrict__ cn, int B, int T, LstmSync sy) {
  constexpr int KL = H / 64, R = 4 * LP_U, G4 = 4 * H;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int u0 = blockIdx.x * LP_U, k0 = lane * KL;
  float w[R][KL];
#pragma unroll
  for (int rr = 0; rr < R; ++rr)
#pragma unroll
    for (int i = 0; i < KL; i += 4) {
      const float4 v4 = *reinterpret_cast<const float4*>(whh + (long)((rr / LP_U) * H + u0 + rr % LP_U) * H + k0 + i);
      w[rr][i] = v4.x; w[rr][i + 1] = v4.y; w[rr][i + 2] = v4.z; w[rr][i + 3] = v4.w;
    }
  // cell lanes: lane = c * 16 + u (gate 0 of unit u of clip c); the other gates at lane + 4q
  const bool cell = (lane & 12) == 0;
  const int cu = lane & 3, k = u0 + cu;
  float bi[4], bh[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    bi[q] = bih[q * H + k];
    bh[q] = bhh[q * H + k];
  }
  const int npass = (B + 15) / 16;
  float cstate[2] = {0.f, 0.f}, hst[2] = {0.f, 0.f}, xq[2][4];
  const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc(out, (short)0, 0x7fffffff, LP_CSP);
  auto clip = [&](int p, int c) { return p * 16 + wv * 4 + c; };
  auto load_xp = [&](int t) {   // x W_ih^T of step t for this lane's cell (prefetched a step ahead; clamped)
    const int tt = min(t, T - 1);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int b = min(clip(p, lane >> 4), B - 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) xq[p][q] = xproj[((long)b * T + tt) * G4 + q * H + k];
    }
  };
  load_xp(0);
  for (int t = 0; t < T; ++t) {
    float xc[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) xc[p][q] = xq[p][q];
    load_xp(t + 1);
    if (t > 0 && !lp_wait(sy, (unsigned)t)) return;
    for (int p = 0; p < npass; ++p) {
      float hv[4][KL];
      if (t > 0) {   // h_{t-1} of the wave's 4 clips (clamped), every 16-B sc1 load issued before any use
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int b = min(clip(p, c), B - 1);
#pragma unroll
          for (int i = 0; i < KL; i += 4) {
            const float4 v4 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                rO, (int)((((long)b * T + t - 1) * H + k0 + i) * 4), 0, LP_SC1));
            hv[c][i] = v4.x; hv[c][i + 1] = v4.y; hv[c][i + 2] = v4.z; hv[c][i + 3] = v4.w;
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int i = 0; i < KL; ++i) hv[c][i] = 0.f;
      }
      float part[4 * R];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
          float a0 = 0.f, a1 = 0.f;
#pragma unroll
          for (int i = 0; i < KL; i += 2) {
            a0 = fmaf(w[rr][i], hv[c][i], a0);
            a1 = fmaf(w[rr][i + 1], hv[c][i + 1], a1);
          }
          part[c * R + rr] = a0 + a1;
        }
      const float rec = lp_rscatter(part, lane);   // clip lane >> 4, row lane & 15
      float pre[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) pre[q] = __shfl(rec, (lane & ~15) | (q * 4 + cu), 64);
      const int b = clip(p, lane >> 4);
      if (cell && b < B) {
        float g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = ((pre[q] + xc[p][q]) + bi[q]) + bh[q];
        const float ig = sigm(g[0]), fg = sigm(g[1]), gg = tanhf(g[2]), og = sigm(g[3]);
        const float c = fmaf(fg, cstate[p], ig * gg);
        const float h = og * tanhf(c);
        const long ob = ((long)b * T + t) * H;
        float* gt = gates + ((long)b * T + t) * G4;
        gt[k] = ig; gt[H + k] = fg; gt[2 * H + k] = gg; gt[3 * H + k] = og;
        hprev[ob + k] = hst[p];
        cst[ob + k] = c;
        lp_st(out + ob + k, h);
        if (t == T - 1) {
          hn[(long)b * H + k] = h;
          cn[(long)b * H + k] = c;
        }
        cstate[p] = c;
        hst[p] = h;
      }
    }
    if (t + 1 < T) lp_publish(sy);
  }
}

// Backward: dh_t[b][k] = dout + sum_j dgates_{t+1}[b][j] W_hh[j][k] needs every gate row j, so instead of
// gathering dgates_{t+1} (B x 4H floats) into every workgroup, each workgroup turns ITS 16 rows'
// dgates into a partial of dh for all H units -- lane l: part[b][k = l*KL .. +KL) = sum over its rows
// of dgates[b][row] W_hh[row][k] (the forward's W slice, the row values broadcast from the cell lanes
// by readlane) -- and publishes it (4 KB per clip, sc1); the next step gathers its 4 units' columns
// of the G partials (16 B per clip and producer) and reduces them over the wave.  Per step and
// workgroup: B x H x 4 B out and B x 16 x G B in (at B = 16, 32 KB each way) instead of B x 4H x 4 B in.
// part: [2 (step parity)][B][H / 4 (unit group)][G (producer)][4] fp32 (the caller's work buffer): a reader's
// gather (its unit group, every producer) is one contiguous 16 x G-byte run per clip, the writes are 16-B
// pieces G x 16 B apart (fire-and-forget; only the publish waits for them).
template <int H>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void lstm_bwd_persist_kernel(const float* __restrict__ dout, const float* __restrict__ dhn,
                             const float* __restrict__ dcn, const float* __restrict__ whh,
                             const float* __restrict__ cst, const float* __restrict__ gates,
                             float* __restrict__ dgates, float* part, int B, int T, LstmSync sy) {
  constexpr int KL = H / 64, R = 4 * LP_U, G4 = 4 * H;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, G = gridDim.x;
  const int u0 = blockIdx.x * LP_U, k0 = lane * KL;
  float w[R][KL];   // W_hh[gate q, unit u0 + u][k0 .. k0+KL), row rr = q * 4 + u
#pragma unroll
  for (int rr = 0; rr < R; ++rr)
#pragma unroll
    for (int i = 0; i < KL; i += 4) {
      const float4 v4 = *reinterpret_cast<const float4*>(whh + (long)((rr / LP_U) * H + u0 + rr % LP_U) * H + k0 + i);
      w[rr][i] = v4.x; w[rr][i + 1] = v4.y; w[rr][i + 2] = v4.z; w[rr][i + 3] = v4.w;
    }
  // cell lanes: lane = c * 16 + u * 4 (clip c of the wave, unit u)
  const bool cell = (lane & 3) == 0;
  const int cu = (lane >> 2) & 3, k = u0 + cu;
  const int npass = (B + 15) / 16;
  const long pstride = (long)G * B * H;   // one parity's partials
  float carry[2] = {0.f, 0.f};
  const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc(part, (short)0, 0x7fffffff, LP_CSP);
  auto clip = [&](int p, int c) { return p * 16 + wv * 4 + c; };
  for (int t = T - 1; t >= 0; --t) {
    const bool last = t == T - 1;
    // this step's cell operands (independent of the recurrence: loaded before the wait; clamped
    // addresses, absent operands selected away)
    float vc[2], vcp[2], vg[2][4], vdo[2], vhn[2], vcn[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int b = min(clip(p, lane >> 4), B - 1);
      const long ob = ((long)b * T + t) * H + k, bk = (long)b * H + k;
      vc[p] = cst[ob];
      vcp[p] = cst[t > 0 ? ob - H : ob];
      vdo[p] = *(dout ? dout + ob : cst + ob);
      vhn[p] = *(dhn ? dhn + bk : cst + ob);
      vcn[p] = *(dcn ? dcn + bk : cst + ob);
#pragma unroll
      for (int q = 0; q < 4; ++q) vg[p][q] = gates[((long)b * T + t) * G4 + q * H + k];
      if (t == 0) vcp[p] = 0.f;
      if (!dout) vdo[p] = 0.f;
      if (!dhn) vhn[p] = 0.f;
      if (!dcn) vcn[p] = 0.f;
    }
    if (!last && !lp_wait(sy, (unsigned)(T - 1 - t))) return;
    for (int p = 0; p < npass; ++p) {
      if (clip(p, 0) >= B) continue;   // (wave-uniform: no clip of this wave in this pass)
      float red[4 * LP_U];
      if (!last) {   // this workgroup's 4 units of the G partials of step t+1: lanes l and l + 64
        const float* pp = part + (long)((t + 1) & 1) * pstride;
        float4 pv[4][2];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int b = min(clip(p, c), B - 1);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int src = min(lane + 64 * e, G - 1);
            pv[c][e] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                rP, (int)((((long)((t + 1) & 1) * pstride + (((long)b * (H / 4) + blockIdx.x) * G + src) * 4) * 4)), 0,
                LP_SC1));
          }
        }
        (void)pp;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bool e1 = lane + 64 < G;
          red[c * 4 + 0] = pv[c][0].x + (e1 ? pv[c][1].x : 0.f);
          red[c * 4 + 1] = pv[c][0].y + (e1 ? pv[c][1].y : 0.f);
          red[c * 4 + 2] = pv[c][0].z + (e1 ? pv[c][1].z : 0.f);
          red[c * 4 + 3] = pv[c][0].w + (e1 ? pv[c][1].w : 0.f);
          if (lane >= G) red[c * 4] = red[c * 4 + 1] = red[c * 4 + 2] = red[c * 4 + 3] = 0.f;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4 * LP_U; ++q) red[q] = 0.f;
      }
      const float rec = lp_rscatter(red, lane);   // clip lane >> 4, unit (lane >> 2) & 3
      const int b = clip(p, lane >> 4);
      float dg[4] = {0.f, 0.f, 0.f, 0.f};
      if (cell && b < B) {
        const float ig = vg[p][0], fg = vg[p][1], gg = vg[p][2], og = vg[p][3];
        const float dhr = !last ? rec : vhn[p];
        const float dcr = !last ? carry[p] : vcn[p];
        const float dh = dhr + vdo[p];
        const float tc = tanhf(vc[p]);
        const float dO = dh * tc;
        const float dc = dcr + dh * og * (1.f - tc * tc);
        const float dI = dc * gg, dG = dc * ig, dF = dc * vcp[p];
        carry[p] = dc * fg;
        dg[0] = dI * ig * (1.f - ig);
        dg[1] = dF * fg * (1.f - fg);
        dg[2] = dG * (1.f - gg * gg);
        dg[3] = dO * og * (1.f - og);
        float* dgo = dgates + ((long)b * T + t) * G4;
#pragma unroll
        for (int q = 0; q < 4; ++q) dgo[q * H + k] = dg[q];
      }
      if (t > 0) {   // this workgroup's partial of dh_{t-1} for the wave's clips, every unit k0 .. k0+KL
        float* pw = part + (long)(t & 1) * pstride + (long)blockIdx.x * B * H;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int bc = clip(p, c);
          float acc[KL];
#pragma unroll
          for (int i = 0; i < KL; ++i) acc[i] = 0.f;
#pragma unroll
          for (int rr = 0; rr < R; ++rr) {   // dgates[bc][gate q, unit u] from cell lane c * 16 + u * 4
            const float d = __builtin_bit_cast(float, __builtin_amdgcn_readlane(
                __builtin_bit_cast(int, dg[rr / LP_U]), c * 16 + (rr % LP_U) * 4));
#pragma unroll
            for (int i = 0; i < KL; ++i) acc[i] = fmaf(d, w[rr][i], acc[i]);
          }
          if (bc < B) {   // units k0 + i .. +3 = unit group (k0 + i) / 4 of this producer
#pragma unroll
            for (int i = 0; i < KL; i += 4)
              __builtin_amdgcn_raw_buffer_store_b128(
                  __builtin_bit_cast(i32x4v, make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3])), rP,
                  (int)(((long)(t & 1) * pstride + (((long)bc * (H / 4) + (k0 + i) / 4) * G + blockIdx.x) * 4) * 4), 0,
                  LP_SC1);
          }
          (void)pw;
        }
      }
    }
    if (t > 0) lp_publish(sy);
  }
}

// Backward, gather form (XCP_LSTM_BWD=gather): each workgroup keeps its 4 units' COLUMNS of W_hh (lane l:
// rows j = l*JL .. +JL, JL = 4H / 64) and gathers the whole dgates_{t+1} of its wave's 4 clips each step
// (every 16-B sc1 load of the step issued before the first use: 512-register waves); per-lane FMA chains,
// reduce-scatter over the wave; it publishes only its own dgates_t (16 floats per clip).
template <int H>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void lstm_bwd_gather_kernel(const float* __restrict__ dout, const float* __restrict__ dhn,
                            const float* __restrict__ dcn, const float* __restrict__ whh,
                            const float* __restrict__ cst, const float* __restrict__ gates, float* dgates, int B,
                            int T, LstmSync sy) {
  constexpr int JL = 4 * H / 64, G4 = 4 * H;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int u0 = blockIdx.x * LP_U, j0 = lane * JL;
  float w[JL][LP_U];
#pragma unroll
  for (int i = 0; i < JL; ++i) {
    const float4 v4 = *reinterpret_cast<const float4*>(whh + (long)(j0 + i) * H + u0);
    w[i][0] = v4.x; w[i][1] = v4.y; w[i][2] = v4.z; w[i][3] = v4.w;
  }
  const bool cell = (lane & 3) == 0;   // lane = c * 16 + u * 4 (clip c, unit u)
  const int cu = (lane >> 2) & 3, k = u0 + cu;
  const int npass = (B + 15) / 16;
  float carry[2] = {0.f, 0.f};
  const __amdgpu_buffer_rsrc_t rG = __builtin_amdgcn_make_buffer_rsrc(dgates, (short)0, 0x7fffffff, LP_CSP);
  auto clip = [&](int p, int c) { return p * 16 + wv * 4 + c; };
  for (int t = T - 1; t >= 0; --t) {
    const bool last = t == T - 1;
    float vc[2], vcp[2], vg[2][4], vdo[2], vhn[2], vcn[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int b = min(clip(p, lane >> 4), B - 1);
      const long ob = ((long)b * T + t) * H + k, bk = (long)b * H + k;
      vc[p] = cst[ob];
      vcp[p] = cst[t > 0 ? ob - H : ob];
      vdo[p] = *(dout ? dout + ob : cst + ob);
      vhn[p] = *(dhn ? dhn + bk : cst + ob);
      vcn[p] = *(dcn ? dcn + bk : cst + ob);
#pragma unroll
      for (int q = 0; q < 4; ++q) vg[p][q] = gates[((long)b * T + t) * G4 + q * H + k];
      if (t == 0) vcp[p] = 0.f;
      if (!dout) vdo[p] = 0.f;
      if (!dhn) vhn[p] = 0.f;
      if (!dcn) vcn[p] = 0.f;
    }
    if (!last && !lp_wait(sy, (unsigned)(T - 1 - t))) return;
    for (int p = 0; p < npass; ++p) {
      if (clip(p, 0) >= B) continue;   // (wave-uniform)
      float part[4 * LP_U];
      if (!last) {
        float dg[4][JL];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int b = min(clip(p, c), B - 1);
#pragma unroll
          for (int i = 0; i < JL; i += 4) {
            const float4 v4 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                rG, (int)((((long)b * T + t + 1) * G4 + j0 + i) * 4), 0, LP_SC1));
            dg[c][i] = v4.x; dg[c][i + 1] = v4.y; dg[c][i + 2] = v4.z; dg[c][i + 3] = v4.w;
          }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int u = 0; u < LP_U; ++u) {
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int i = 0; i < JL; i += 2) {
              a0 = fmaf(dg[c][i], w[i][u], a0);
              a1 = fmaf(dg[c][i + 1], w[i + 1][u], a1);
            }
            part[c * LP_U + u] = a0 + a1;
          }
      } else {
#pragma unroll
        for (int q = 0; q < 4 * LP_U; ++q) part[q] = 0.f;
      }
      const float rec = lp_rscatter(part, lane);   // clip lane >> 4, unit (lane >> 2) & 3
      const int b = clip(p, lane >> 4);
      if (cell && b < B) {
        const float ig = vg[p][0], fg = vg[p][1], gg = vg[p][2], og = vg[p][3];
        const float dhr = !last ? rec : vhn[p];
        const float dcr = !last ? carry[p] : vcn[p];
        const float dh = dhr + vdo[p];
        const float tc = tanhf(vc[p]);
        const float dO = dh * tc;
        const float dc = dcr + dh * og * (1.f - tc * tc);
        const float dI = dc * gg, dG = dc * ig, dF = dc * vcp[p];
        carry[p] = dc * fg;
        float* dgo = dgates + ((long)b * T + t) * G4;
        lp_st(dgo + k, dI * ig * (1.f - ig));
        lp_st(dgo + H + k, dF * fg * (1.f - fg));
        lp_st(dgo + 2 * H + k, dG * (1.f - gg * gg));
        lp_st(dgo + 3 * H + k, dO * og * (1.f - og));
      }
    }
    if (t > 0) lp_publish(sy);
  }
}

// Backward, clip-grouped gather form (XCP_LSTM_BWD=cg / cg2): the gather kernel's workgroups split by clips as
// well -- workgroup (unit group ug, clip group cg) keeps its 4 units' columns of W_hh and each of its 4
// waves gathers CPW clips' dgates_{t+1} (8 CPW 16-B sc1 loads per lane instead of 32), at H / 4 x
// ceil(B / (4 CPW)) workgroups (CPW 1: two per CU at B = 16, H = 512 -- 128-VGPR weights + one clip's 32
// dgates per lane fit the 256 registers of two waves per SIMD; CPW 2: one per CU).  CPW = 4 with one clip
// group is the gather kernel.
// Per-lane partial chains, reduce-scatter tree and cell update are the gather kernel's, so dgates are
// bitwise its.
template <int H, int CPW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CPW == 1 ? 2 : 1, CPW == 1 ? 2 : 1)))
void lstm_bwd_cg_kernel(const float* __restrict__ dout, const float* __restrict__ dhn,
                        const float* __restrict__ dcn, const float* __restrict__ whh,
                        const float* __restrict__ cst, const float* __restrict__ gates, float* dgates, int B,
                        int T, LstmSync sy) {
  constexpr int JL = 4 * H / 64, G4 = 4 * H, NG = H / LP_U, NP = CPW * LP_U;
  constexpr int SH = CPW == 1 ? 4 : CPW == 2 ? 3 : 2;   // lane >> SH: index c * LP_U + u after the reduce-scatter
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ug = blockIdx.x % NG, cgp = blockIdx.x / NG;
  const int u0 = ug * LP_U, j0 = lane * JL;
  float w[JL][LP_U];
#pragma unroll
  for (int i = 0; i < JL; ++i) {
    const float4 v4 = *reinterpret_cast<const float4*>(whh + (long)(j0 + i) * H + u0);
    w[i][0] = v4.x; w[i][1] = v4.y; w[i][2] = v4.z; w[i][3] = v4.w;
  }
  // this wave's clips (cgp * 4 + wv) * CPW + c; clips past B idle, but keep every barrier
  const int cb = (cgp * 4 + wv) * CPW;
  const int idx = lane >> SH;
  const bool cell = (lane & ((1 << SH) - 1)) == 0;   // lane = (c * LP_U + u) << SH
  const int b = cb + idx / LP_U, k = u0 + idx % LP_U;
  const bool bok = b < B;
  const int bb = bok ? b : B - 1;
  float carry = 0.f;
  const __amdgpu_buffer_rsrc_t rG = __builtin_amdgcn_make_buffer_rsrc(dgates, (short)0, 0x7fffffff, LP_CSP);
  for (int t = T - 1; t >= 0; --t) {
    const bool last = t == T - 1;
    const long ob = ((long)bb * T + t) * H + k, bk = (long)bb * H + k;
    const float vc = cst[ob];
    float vcp = cst[t > 0 ? ob - H : ob];
    float vdo = *(dout ? dout + ob : cst + ob);
    float vhn = *(dhn ? dhn + bk : cst + ob);
    float vcn = *(dcn ? dcn + bk : cst + ob);
    float vg[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) vg[q] = gates[((long)bb * T + t) * G4 + q * H + k];
    if (t == 0) vcp = 0.f;
    if (!dout) vdo = 0.f;
    if (!dhn) vhn = 0.f;
    if (!dcn) vcn = 0.f;
    if (!last && !lp_wait(sy, (unsigned)(T - 1 - t))) return;
    float part[NP];
    if (!last) {
      float dg[CPW][JL];
#pragma unroll
      for (int c = 0; c < CPW; ++c) {
        const int bc = min(cb + c, B - 1);
#pragma unroll
        for (int i = 0; i < JL; i += 4) {
          const float4 v4 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
              rG, (int)((((long)bc * T + t + 1) * G4 + j0 + i) * 4), 0, LP_SC1));
          dg[c][i] = v4.x; dg[c][i + 1] = v4.y; dg[c][i + 2] = v4.z; dg[c][i + 3] = v4.w;
        }
      }
#pragma unroll
      for (int c = 0; c < CPW; ++c)
#pragma unroll
        for (int u = 0; u < LP_U; ++u) {
          float a0 = 0.f, a1 = 0.f;
#pragma unroll
          for (int i = 0; i < JL; i += 2) {
            a0 = fmaf(dg[c][i], w[i][u], a0);
            a1 = fmaf(dg[c][i + 1], w[i + 1][u], a1);
          }
          part[c * LP_U + u] = a0 + a1;
        }
    } else {
#pragma unroll
      for (int q = 0; q < NP; ++q) part[q] = 0.f;
    }
    const float rec = lp_rscatter(part, lane);   // index lane >> SH
    if (cell && bok) {
      const float ig = vg[0], fg = vg[1], gg = vg[2], og = vg[3];
      const float dhr = !last ? rec : vhn;
      const float dcr = !last ? carry : vcn;
      const float dh = dhr + vdo;
      const float tc = tanhf(vc);
      const float dO = dh * tc;
      const float dc = dcr + dh * og * (1.f - tc * tc);
      const float dI = dc * gg, dG = dc * ig, dF = dc * vcp;
      carry = dc * fg;
      float* dgo = dgates + ((long)b * T + t) * G4;
      lp_st(dgo + k, dI * ig * (1.f - ig));
      lp_st(dgo + H + k, dF * fg * (1.f - fg));
      lp_st(dgo + 2 * H + k, dG * (1.f - gg * gg));
      lp_st(dgo + 3 * H + k, dO * og * (1.f - og));
    }
    if (t > 0) lp_publish(sy);
  }
}

__device__ unsigned g_lstm_sync[64][8 * LP_SHARD + 32];   // per (device, stream) slot: shards, error word

// Kernel choice (`kernel` argument: 0 = auto, 1 = the generic kernels, used by tests to pin
// them at shapes the specialised kernels also cover).
// register-resident: one 1024-thread workgroup per clip, W_hh slice in VGPRs
bool lstm_reg(int H, int kernel) { return kernel == 0 && (H == 128 || H == 64); }
// per-step kernels: H = 32 * KS for the instantiated KS, clips within the register partials
bool lstm_step(int B, int H, int kernel) {
  const size_t fwd_lds = ((size_t)B * 32 * (H / 32 + 4) + 8 * B) * sizeof(float);
  const size_t bwd_lds = ((size_t)8 * H + 64 + 2 * B) * sizeof(float);
  return kernel == 0 && !lstm_reg(H, kernel) && (H == 256 || H == 512 || H == 1024) && B <= LS_MAXB &&
         fwd_lds <= 65536 && bwd_lds <= 65536;
}

// persistent kernels for H = 256 / 512, B <= 32, when all G = H / 4 workgroups can be resident at once (the
// occupancy query).  Default: the forward only -- at XceptionLSTMA's shape (B 16, T 120, H 512) it runs 4.6 us
// per step against the per-step kernels' 6.3; the persistent backward (published dh partials) is faster at
// small B (3.9 vs 4.6 us per step at B 2) but slower at B 16 (9.5 vs 7.3: the partials' sc1 traffic), so the
// per-step backward stays there (profiles/r06_lstm_ab.txt); where the clip-grouped backward's workgroups take
// at most half the CUs it is the default (xcp_lstm_bwd).  XCP_LSTM_PERSIST=0: neither, 1: both (read per call).
int lstm_persist_mode() {
  const char* e = getenv("XCP_LSTM_PERSIST");
  return e && e[0] == '0' ? 0 : e && e[0] == '1' ? 2 : 1;
}
bool lstm_persist_env(bool fwd) { return lstm_persist_mode() >= (fwd ? 1 : 2); }
bool lstm_bwd_gather() {   // XCP_LSTM_BWD=gather: the persistent backward's gather form (A/B; read per call)
  const char* e = getenv("XCP_LSTM_BWD");
  return e && e[0] == 'g';
}
int lstm_bwd_cg() {   // XCP_LSTM_BWD=cg / cg2: the clip-grouped gather form, 1 / 2 clips per wave (A/B; read per call)
  const char* e = getenv("XCP_LSTM_BWD");
  if (!(e && e[0] == 'c' && e[1] == 'g')) return 0;
  return e[2] == '2' ? 2 : 1;
}
bool lstm_cg_default(int B, int H, int kernel) {
  return kernel == 0 && B <= 32 && (H == 256 || H == 512) && lstm_persist_mode() == 1 && !getenv("XCP_LSTM_BWD");
}
int lp_cus() {
  static const int v = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return 0;
    return n;
  }();
  return v;
}
template <typename K>
bool lp_resident(K kern, int G) {
  int dev = 0, cus = 0, per = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return false;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, 256, 0) != hipSuccess) return false;
  return (long)per * cus >= G;
}
bool lstm_persist(int B, int H, int kernel, bool fwd) {
  if (kernel != 0 || B > 32 || !(H == 256 || H == 512) || !lstm_persist_env(fwd)) return false;
  static int ok[2][2] = {{-1, -1}, {-1, -1}};   // [fwd][H == 512]
  int& v = ok[fwd][H == 512];
  if (v < 0) {
    if (fwd) v = H == 512 ? lp_resident(lstm_fwd_persist_kernel<512>, H / LP_U) : lp_resident(lstm_fwd_persist_kernel<256>, H / LP_U);
    else v = H == 512 ? lp_resident(lstm_bwd_persist_kernel<512>, H / LP_U) : lp_resident(lstm_bwd_persist_kernel<256>, H / LP_U);
  }
  return v == 1;
}

// the sync words of (device, stream), zeroed on the stream before each persistent launch
int lp_sync(hipStream_t st, LstmSync& sy) {
  static std::mutex mu;
  static std::vector<std::pair<int, hipStream_t>> slots;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return XCP_EINVAL;
  int slot = -1;
  {
    std::lock_guard<std::mutex> lk(mu);
    for (size_t i = 0; i < slots.size(); ++i)
      if (slots[i].first == dev && slots[i].second == st) slot = (int)i;
    if (slot < 0) {
      if (slots.size() >= 64) return XCP_EUNSUPPORTED;
      slots.emplace_back(dev, st);
      slot = (int)slots.size() - 1;
    }
  }
  void* base = nullptr;
  if (hipGetSymbolAddress(&base, HIP_SYMBOL(g_lstm_sync)) != hipSuccess) return XCP_EINVAL;
  unsigned* words = reinterpret_cast<unsigned*>(base) + (long)slot * (8 * LP_SHARD + 32);
  if (hipMemsetAsync(words, 0, 8 * LP_SHARD * sizeof(unsigned), st) != hipSuccess) return XCP_EINVAL;
  sy.cnt = words;
  sy.err = words + 8 * LP_SHARD;
  return XCP_OK;
}

// Forward and backward dispatch.  lens null: fixed length; non-null: per-clip lengths, which skip
// the persistent, clip-grouped and gather kernels (those have no length-aware form).
bool lstm_fwd_persist(int B, int H, int kernel, bool vl) { return !vl && lstm_persist(B, H, kernel, true); }

// the register-resident, per-step or generic forward (ST: from the state h0 / c0 [B][H], both non-null)
template <bool VL, bool ST = false>
int lstm_fwd_launch(const float* xproj, const float* whh, const float* whhT, const float* bih, const float* bhh, float* out,
                    float* hprev, float* cst, float* gates, float* hn, float* cn, const int* lens, int B, int T, int H,
                    int kernel, hipStream_t st, const float* h0 = nullptr, const float* c0 = nullptr) {
  if (lstm_reg(H, kernel)) {
    if (H == 128)
      hipLaunchKernelGGL((lstm_fwd_reg_kernel<128, VL, ST>), dim3(B), dim3(1024), 0, st, xproj, whh, bih, bhh, out,
                         hprev, cst, gates, hn, cn, T, lens, h0, c0, LstmDirs{});
    else
      hipLaunchKernelGGL((lstm_fwd_reg_kernel<64, VL, ST>), dim3(B), dim3(1024), 0, st, xproj, whh, bih, bhh, out,
                         hprev, cst, gates, hn, cn, T, lens, h0, c0, LstmDirs{});
    return (int)hipGetLastError();
  }
  if (lstm_step(B, H, kernel)) {
    const size_t smem = ((size_t)B * 32 * (H / 32 + 4) + 8 * B) * sizeof(float);
    for (int t = 0; t < T; ++t) {
      if (H == 256)
        hipLaunchKernelGGL((lstm_fwd_step_kernel<8, VL, ST>), dim3(H / LS_UPW), dim3(256), smem, st, xproj, whh, bih,
                           bhh, out, hprev, cst, gates, hn, cn, B, T, t, lens, h0, c0, LstmDirs{});
      else if (H == 512)
        hipLaunchKernelGGL((lstm_fwd_step_kernel<16, VL, ST>), dim3(H / LS_UPW), dim3(256), smem, st, xproj, whh, bih,
                           bhh, out, hprev, cst, gates, hn, cn, B, T, t, lens, h0, c0, LstmDirs{});
      else
        hipLaunchKernelGGL((lstm_fwd_step_kernel<32, VL, ST>), dim3(H / LS_UPW), dim3(256), smem, st, xproj, whh, bih,
                           bhh, out, hprev, cst, gates, hn, cn, B, T, t, lens, h0, c0, LstmDirs{});
    }
    return (int)hipGetLastError();
  }
  if (!whhT) return XCP_EINVAL;
  const size_t smem = (size_t)6 * H * sizeof(float);
  hipLaunchKernelGGL((lstm_fwd_kernel<VL, ST>), dim3(B), dim3(256), smem, st, xproj, whhT, bih, bhh, out, hprev, cst,
                     gates, hn, cn, T, H, lens, h0, c0, LstmDirs{});
  return (int)hipGetLastError();
}

int lstm_fwd(const float* xproj, const float* whh, const float* whhT, const float* bih, const float* bhh, float* out,
             float* hprev, float* cst, float* gates, float* hn, float* cn, const int* lens, int B, int T, int H, int kernel,
             hipStream_t st) {
  if (B <= 0 || T <= 0) return XCP_OK;
  if (kernel < 0 || kernel > 1) return XCP_EINVAL;
  if (lstm_fwd_persist(B, H, kernel, lens != nullptr)) {
    LstmSync sy;
    const int rc = lp_sync(st, sy);
    if (rc != XCP_OK) return rc;
    if (H == 512)
      hipLaunchKernelGGL(lstm_fwd_persist_kernel<512>, dim3(H / LP_U), dim3(256), 0, st, xproj, whh, bih, bhh, out, hprev,
                         cst, gates, hn, cn, B, T, sy);
    else
      hipLaunchKernelGGL(lstm_fwd_persist_kernel<256>, dim3(H / LP_U), dim3(256), 0, st, xproj, whh, bih, bhh, out, hprev,
                         cst, gates, hn, cn, B, T, sy);
    return (int)hipGetLastError();
  }
  return lens ? lstm_fwd_launch<true>(xproj, whh, whhT, bih, bhh, out, hprev, cst, gates, hn, cn, lens, B, T, H, kernel, st)
              : lstm_fwd_launch<false>(xproj, whh, whhT, bih, bhh, out, hprev, cst, gates, hn, cn, lens, B, T, H, kernel, st);
}

// 1 when lstm_fwd (same B, H, kernel; vl: with lengths) runs the generic kernel, which reads the transposed W_hh
// (the register-resident, persistent and per-step forward kernels read W_hh as stored)
int lstm_needs_whhT(int B, int H, int kernel, bool vl) {
  return lstm_reg(H, kernel) || lstm_fwd_persist(B, H, kernel, vl) || lstm_step(B, H, kernel) ? 0 : 1;
}

// the per-step, register-resident or generic backward (ST: step 0 takes c0 [B][H] (null: zero) as c_{-1}, and
// dh0 / dc0 [B][H], each nullable, receive the state's gradient; the per-step form spends one more launch
// on them, which runs the recurrent sum over dgates_0 alone)
template <bool VL, bool ST = false>
int lstm_bwd_launch(const float* dout, const float* dhn, const float* dcn, const float* whh, const float* cst,
                    const float* gates, float* dgates, float* work, const int* lens, int B, int T, int H, int kernel,
                    hipStream_t st, const float* c0 = nullptr, float* dh0 = nullptr, float* dc0 = nullptr) {
  if (lstm_step(B, H, kernel)) {
    if (!work) return XCP_EINVAL;
    float* whhT = work + (long)B * H;
    hipLaunchKernelGGL(lstm_transpose_kernel, dim3(4 * H / 32, H / 32), dim3(256), 0, st, whh, whhT, H);
    const size_t smem = ((size_t)8 * H + 64 + 2 * B) * sizeof(float);
    for (int t = T - 1; t >= (ST && (dh0 || dc0) ? -1 : 0); --t)
      hipLaunchKernelGGL((lstm_bwd_step_kernel<VL, ST>), dim3(H / LS_UPW), dim3(256), smem, st, dout, dhn, dcn, whhT, cst,
                         gates, dgates, work, B, T, H, t, lens, c0, dh0, dc0, LstmDirs{});
    return (int)hipGetLastError();
  }
  if (lstm_reg(H, kernel)) {
    if (H == 128)
      hipLaunchKernelGGL((lstm_bwd_reg_kernel<128, VL, ST>), dim3(B), dim3(1024), 0, st, dout, dhn, dcn, whh, cst, gates,
                         dgates, T, lens, c0, dh0, dc0, LstmDirs{});
    else
      hipLaunchKernelGGL((lstm_bwd_reg_kernel<64, VL, ST>), dim3(B), dim3(1024), 0, st, dout, dhn, dcn, whh, cst, gates,
                         dgates, T, lens, c0, dh0, dc0, LstmDirs{});
    return (int)hipGetLastError();
  }
  const size_t smem = (size_t)6 * H * sizeof(float);
  hipLaunchKernelGGL((lstm_bwd_kernel<VL, ST>), dim3(B), dim3(256), smem, st, dout, dhn, dcn, whh, cst, gates, dgates, T,
                     H, lens, c0, dh0, dc0, LstmDirs{});
  return (int)hipGetLastError();
}

int lstm_bwd(const float* dout, const float* dhn, const float* dcn, const float* whh, const float* cst, const float* gates,
             float* dgates, float* work, const int* lens, int B, int T, int H, int kernel, hipStream_t st) {
  if (B <= 0 || T <= 0) return XCP_OK;
  if (kernel < 0 || kernel > 1) return XCP_EINVAL;
  const bool fixed = !lens;   // only a fixed-length call takes the persistent forms
  // clip-grouped form: cpw clips per wave, H / 4 x ceil(B / (4 cpw)) workgroups, if they can all be resident
  auto cg_grid = [&](int cpw) { return (H / LP_U) * ((B + 4 * cpw - 1) / (4 * cpw)); };
  auto cg_fits = [&](int cpw) {
    const int g = cg_grid(cpw);
    if (cpw == 1) return H == 512 ? lp_resident(lstm_bwd_cg_kernel<512, 1>, g) : lp_resident(lstm_bwd_cg_kernel<256, 1>, g);
    return H == 512 ? lp_resident(lstm_bwd_cg_kernel<512, 2>, g) : lp_resident(lstm_bwd_cg_kernel<256, 2>, g);
  };
  auto launch_cg = [&](int cpw) {
    LstmSync sy;
    const int rc = lp_sync(st, sy);
    if (rc != XCP_OK) return rc;
    const dim3 g(cg_grid(cpw));
#define XCP_LCG(HH, C) hipLaunchKernelGGL((lstm_bwd_cg_kernel<HH, C>), g, dim3(256), 0, st, dout, dhn, dcn, whh, cst, gates, dgates, B, T, sy)
    if (H == 512 && cpw == 1) XCP_LCG(512, 1);
    else if (H == 512) XCP_LCG(512, 2);
    else if (cpw == 1) XCP_LCG(256, 1);
    else XCP_LCG(256, 2);
#undef XCP_LCG
    return (int)hipGetLastError();
  };
  // default (XCP_LSTM_PERSIST and XCP_LSTM_BWD unset): the clip-grouped persistent backward where its workgroups
  // take at most half the CUs, as the persistent forward's do (H = 512 up to 4 clips, H = 256 up to 8): 30-47 %
  // faster than the per-step kernels there.  Elsewhere the per-step kernels: at XceptionLSTMA's B 16 x H 512 the
  // two-clips-per-wave form (XCP_LSTM_BWD=cg2) is 2 % faster but needs every CU resident at once
  // (profiles/r06_lstm_cg_ab.txt)
  if (fixed && lstm_cg_default(B, H, kernel) && 2 * cg_grid(1) <= lp_cus() && cg_fits(1)) return launch_cg(1);
  if (fixed && lstm_persist(B, H, kernel, false)) {
    const int cpw = lstm_bwd_cg();
    if (cpw && cg_fits(cpw)) return launch_cg(cpw);
    LstmSync sy;
    const int rc = lp_sync(st, sy);
    if (rc != XCP_OK) return rc;
    if (lstm_bwd_gather()) {
      if (H == 512)
        hipLaunchKernelGGL(lstm_bwd_gather_kernel<512>, dim3(H / LP_U), dim3(256), 0, st, dout, dhn, dcn, whh, cst, gates,
                           dgates, B, T, sy);
      else
        hipLaunchKernelGGL(lstm_bwd_gather_kernel<256>, dim3(H / LP_U), dim3(256), 0, st, dout, dhn, dcn, whh, cst, gates,
                           dgates, B, T, sy);
      return (int)hipGetLastError();
    }
    if (!work) return XCP_EINVAL;
    if (H == 512)
      hipLaunchKernelGGL(lstm_bwd_persist_kernel<512>, dim3(H / LP_U), dim3(256), 0, st, dout, dhn, dcn, whh, cst, gates,
                         dgates, work, B, T, sy);
    else
      hipLaunchKernelGGL(lstm_bwd_persist_kernel<256>, dim3(H / LP_U), dim3(256), 0, st, dout, dhn, dcn, whh, cst, gates,
                         dgates, work, B, T, sy);
    return (int)hipGetLastError();
  }
  return lens ? lstm_bwd_launch<true>(dout, dhn, dcn, whh, cst, gates, dgates, work, lens, B, T, H, kernel, st)
              : lstm_bwd_launch<false>(dout, dhn, dcn, whh, cst, gates, dgates, work, lens, B, T, H, kernel, st);
}

// Direction-aware forward / backward (the DR instantiations): D = 1 (dirs 1 or 2) or 2 (dirs 3) slots of the
// stacked arrays, both in the same launches -- grid (B, D) for the per-clip families, (H / 2, D) per step.
template <bool VL, bool ST>
int lstm_fwd_dir_launch(const float* xproj, const float* whh, const float* whhT, const float* bih, const float* bhh,
                        const float* h0, const float* c0, float* out, float* hprev, float* cst, float* gates, float* hn,
                        float* cn, const int* lens, int B, int T, int H, int kernel, int dirs, hipStream_t st) {
  const int D = dirs == 3 ? 2 : 1;
  const LstmDirs dd{dirs == 2 ? 1 : 0, D * H};
  if (lstm_reg(H, kernel)) {
    if (H == 128)
      hipLaunchKernelGGL((lstm_fwd_reg_kernel<128, VL, ST, true>), dim3(B, D), dim3(1024), 0, st, xproj, whh, bih, bhh,
                         out, hprev, cst, gates, hn, cn, T, lens, h0, c0, dd);
    else
      hipLaunchKernelGGL((lstm_fwd_reg_kernel<64, VL, ST, true>), dim3(B, D), dim3(1024), 0, st, xproj, whh, bih, bhh,
                         out, hprev, cst, gates, hn, cn, T, lens, h0, c0, dd);
    return (int)hipGetLastError();
  }
  if (lstm_step(B, H, kernel)) {
    const size_t smem = ((size_t)B * 32 * (H / 32 + 4) + 8 * B) * sizeof(float);
    for (int t = 0; t < T; ++t) {
      if (H == 256)
        hipLaunchKernelGGL((lstm_fwd_step_kernel<8, VL, ST, true>), dim3(H / LS_UPW, D), dim3(256), smem, st, xproj, whh,
                           bih, bhh, out, hprev, cst, gates, hn, cn, B, T, t, lens, h0, c0, dd);
      else if (H == 512)
        hipLaunchKernelGGL((lstm_fwd_step_kernel<16, VL, ST, true>), dim3(H / LS_UPW, D), dim3(256), smem, st, xproj, whh,
                           bih, bhh, out, hprev, cst, gates, hn, cn, B, T, t, lens, h0, c0, dd);
      else
        hipLaunchKernelGGL((lstm_fwd_step_kernel<32, VL, ST, true>), dim3(H / LS_UPW, D), dim3(256), smem, st, xproj, whh,
                           bih, bhh, out, hprev, cst, gates, hn, cn, B, T, t, lens, h0, c0, dd);
    }
    return (int)hipGetLastError();
  }
  if (!whhT) return XCP_EINVAL;
  const size_t smem = (size_t)6 * H * sizeof(float);
  hipLaunchKernelGGL((lstm_fwd_kernel<VL, ST, true>), dim3(B, D), dim3(256), smem, st, xproj, whhT, bih, bhh, out, hprev,
                     cst, gates, hn, cn, T, H, lens, h0, c0, dd);
  return (int)hipGetLastError();
}

// work (per-step kernels only): [D][cell-gradient carry B*H, W_hh^T H*4H]
template <bool VL, bool ST>
int lstm_bwd_dir_launch(const float* dout, const float* dhn, const float* dcn, const float* whh, const float* c0,
                        const float* cst, const float* gates, float* dgates, float* dh0, float* dc0, float* work,
                        const int* lens, int B, int T, int H, int kernel, int dirs, hipStream_t st) {
  const int D = dirs == 3 ? 2 : 1;
  const LstmDirs dd{dirs == 2 ? 1 : 0, D * H};
  if (lstm_step(B, H, kernel)) {
    if (!work) return XCP_EINVAL;
    const long ws = (long)B * H + (long)4 * H * H;
    for (int d = 0; d < D; ++d)
      hipLaunchKernelGGL(lstm_transpose_kernel, dim3(4 * H / 32, H / 32), dim3(256), 0, st, whh + (long)d * 4 * H * H,
                         work + d * ws + (long)B * H, H);
    const size_t smem = ((size_t)8 * H + 64 + 2 * B) * sizeof(float);
    for (int t = T - 1; t >= (ST && (dh0 || dc0) ? -1 : 0); --t)
      hipLaunchKernelGGL((lstm_bwd_step_kernel<VL, ST, true>), dim3(H / LS_UPW, D), dim3(256), smem, st, dout, dhn, dcn,
                         work + (long)B * H, cst, gates, dgates, work, B, T, H, t, lens, c0, dh0, dc0, dd);
    return (int)hipGetLastError();
  }
  if (lstm_reg(H, kernel)) {
    if (H == 128)
      hipLaunchKernelGGL((lstm_bwd_reg_kernel<128, VL, ST, true>), dim3(B, D), dim3(1024), 0, st, dout, dhn, dcn, whh, cst,
                         gates, dgates, T, lens, c0, dh0, dc0, dd);
    else
      hipLaunchKernelGGL((lstm_bwd_reg_kernel<64, VL, ST, true>), dim3(B, D), dim3(1024), 0, st, dout, dhn, dcn, whh, cst,
                         gates, dgates, T, lens, c0, dh0, dc0, dd);
    return (int)hipGetLastError();
  }
  const size_t smem = (size_t)6 * H * sizeof(float);
  hipLaunchKernelGGL((lstm_bwd_kernel<VL, ST, true>), dim3(B, D), dim3(256), smem, st, dout, dhn, dcn, whh, cst, gates,
                     dgates, T, H, lens, c0, dh0, dc0, dd);
  return (int)hipGetLastError();
}

}  // namespace


extern "C" {

// 1 when a persistent LSTM launch on any stream gave up waiting for its workgroups (its results are
// invalid); clears the flags.  Synchronises the device.
int xcp_lstm_sync_error() {
  void* base = nullptr;
  if (hipDeviceSynchronize() != hipSuccess || hipGetSymbolAddress(&base, HIP_SYMBOL(g_lstm_sync)) != hipSuccess)
    return -1;
  static unsigned host[64][8 * LP_SHARD + 32];
  if (hipMemcpy(host, base, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  int any = 0;
  for (int i = 0; i < 64; ++i)
    if (host[i][8 * LP_SHARD]) {
      any = 1;
      unsigned* w = reinterpret_cast<unsigned*>(base) + (long)i * (8 * LP_SHARD + 32) + 8 * LP_SHARD;
      if (hipMemset(w, 0, sizeof(unsigned)) != hipSuccess) return -1;
    }
  return any;
}

// 1 when xcp_lstm_fwd (same B, H, kernel) runs the generic kernel, which reads the transposed W_hh
int xcp_lstm_needs_whhT(int B, int H, int kernel) { return lstm_needs_whhT(B, H, kernel, false); }

int xcp_lstm_fwd(const float* xproj, const float* whh, const float* whhT, const float* bih, const float* bhh, float* out,
                 float* hprev, float* cst, float* gates, float* hn, float* cn, int B, int T, int H, int kernel,
                 hipStream_t st) {
  return lstm_fwd(xproj, whh, whhT, bih, bhh, out, hprev, cst, gates, hn, cn, nullptr, B, T, H, kernel, st);
}

int xcp_lstm_bwd(const float* dout, const float* dhn, const float* dcn, const float* whh, const float* cst,
                 const float* gates, float* dgates, float* work, int B, int T, int H, int kernel, hipStream_t st) {
  return lstm_bwd(dout, dhn, dcn, whh, cst, gates, dgates, work, nullptr, B, T, H, kernel, st);
}

// The same with per-clip lengths (lens [B], device memory; null is an error, not "fixed length").
int xcp_lstm_varlen_needs_whhT(int B, int H, int kernel) { return lstm_needs_whhT(B, H, kernel, true); }

int xcp_lstm_fwd_varlen(const float* xproj, const float* whh, const float* whhT, const float* bih, const float* bhh,
                        float* out, float* hprev, float* cst, float* gates, float* hn, float* cn, const int* lens, int B,
                        int T, int H, int kernel, hipStream_t st) {
  if (B > 0 && T > 0 && (H <= 0 || !lens)) return XCP_EINVAL;
  return lstm_fwd(xproj, whh, whhT, bih, bhh, out, hprev, cst, gates, hn, cn, lens, B, T, H, kernel, st);
}

int xcp_lstm_bwd_varlen(const float* dout, const float* dhn, const float* dcn, const float* whh, const float* cst,
                        const float* gates, float* dgates, float* work, const int* lens, int B, int T, int H, int kernel,
                        hipStream_t st) {
  if (B > 0 && T > 0 && (H <= 0 || !lens)) return XCP_EINVAL;
  return lstm_bwd(dout, dhn, dcn, whh, cst, gates, dgates, work, lens, B, T, H, kernel, st);
}

// From an initial state: nn.LSTM(...)(x, (h0, c0)), with lengths (lens non-null) the same over packed input.
// h0 / c0 [B][H] fp32, given together (both null: the plain call above); they must not alias hn / cn.  A call
// with a state takes the register-resident, per-step or generic kernels only -- never one that polls.
int xcp_lstm_state_needs_whhT(int B, int H, int kernel) { return lstm_reg(H, kernel) || lstm_step(B, H, kernel) ? 0 : 1; }

int xcp_lstm_fwd_state(const float* xproj, const float* whh, const float* whhT, const float* bih, const float* bhh,
                       const float* h0, const float* c0, float* out, float* hprev, float* cst, float* gates, float* hn,
                       float* cn, const int* lens, int B, int T, int H, int kernel, hipStream_t st) {
  if ((h0 == nullptr) != (c0 == nullptr)) return XCP_EINVAL;
  if (B <= 0 || T <= 0) return XCP_OK;
  if (H <= 0 || kernel < 0 || kernel > 1) return XCP_EINVAL;
  if (!h0) return lstm_fwd(xproj, whh, whhT, bih, bhh, out, hprev, cst, gates, hn, cn, lens, B, T, H, kernel, st);
  return lens ? lstm_fwd_launch<true, true>(xproj, whh, whhT, bih, bhh, out, hprev, cst, gates, hn, cn, lens, B, T, H,
                                            kernel, st, h0, c0)
              : lstm_fwd_launch<false, true>(xproj, whh, whhT, bih, bhh, out, hprev, cst, gates, hn, cn, lens, B, T, H,
                                             kernel, st, h0, c0);
}

// Backward of the above: c0 [B][H] is step 0's c_{t-1} (null: zero); dh0 / dc0 [B][H] receive d/dh0 and d/dc0
// (each nullable: not wanted).  work as for xcp_lstm_bwd_varlen.
int xcp_lstm_bwd_state(const float* dout, const float* dhn, const float* dcn, const float* whh, const float* c0,
                       const float* cst, const float* gates, float* dgates, float* dh0, float* dc0, float* work,
                       const int* lens, int B, int T, int H, int kernel, hipStream_t st) {
  if (B <= 0 || T <= 0) return XCP_OK;
  if (H <= 0 || kernel < 0 || kernel > 1) return XCP_EINVAL;
  return lens ? lstm_bwd_launch<true, true>(dout, dhn, dcn, whh, cst, gates, dgates, work, lens, B, T, H, kernel, st, c0,
                                            dh0, dc0)
              : lstm_bwd_launch<false, true>(dout, dhn, dcn, whh, cst, gates, dgates, work, lens, B, T, H, kernel, st, c0,
                                             dh0, dc0);
}

// Both directions of time: nn.LSTM(I, H, 1, batch_first=True, bidirectional=True), with lengths (lens non-null)
// over packed input.  dirs is a mask: 1 = the forward direction only, 2 = the reverse one only, 3 = both, with
// D = 1, 1, 2 slots on the leading axis of every stacked array (whh [D][4H][H], whhT [D][H][4H], bih / bhh
// [D][4H], xproj / gates / dgates [D][B*T][4H], hprev / cst [D][B][T][H], h0 / c0 / hn / cn / dh0 / dc0
// [D][B][H]); out / dout are [B][T][D*H], slot d in columns d*H .. d*H + H.  h0 / c0 are nullable together,
// lens is nullable, dh0 / dc0 each.  Runs the register-resident, per-step or generic kernels only -- never one
// that polls -- and both directions in the same launches.  work: D * (B*H + 4*H*H) floats (per-step kernels).
int xcp_lstm_dir_needs_whhT(int B, int H, int kernel) { return lstm_reg(H, kernel) || lstm_step(B, H, kernel) ? 0 : 1; }

int xcp_lstm_fwd_dir(const float* xproj, const float* whh, const float* whhT, const float* bih, const float* bhh,
                     const float* h0, const float* c0, float* out, float* hprev, float* cst, float* gates, float* hn,
                     float* cn, const int* lens, int B, int T, int H, int kernel, int dirs, hipStream_t st) {
  if ((h0 == nullptr) != (c0 == nullptr) || dirs < 1 || dirs > 3) return XCP_EINVAL;
  if (B <= 0 || T <= 0) return XCP_OK;
  if (H <= 0 || kernel < 0 || kernel > 1) return XCP_EINVAL;
#define XCP_LFD(VL, ST) lstm_fwd_dir_launch<VL, ST>(xproj, whh, whhT, bih, bhh, h0, c0, out, hprev, cst, gates, hn, cn, lens, B, T, H, kernel, dirs, st)
  if (h0) return lens ? XCP_LFD(true, true) : XCP_LFD(false, true);
  return lens ? XCP_LFD(true, false) : XCP_LFD(false, false);
#undef XCP_LFD
}

int xcp_lstm_bwd_dir(const float* dout, const float* dhn, const float* dcn, const float* whh, const float* c0,
                     const float* cst, const float* gates, float* dgates, float* dh0, float* dc0, float* work,
                     const int* lens, int B, int T, int H, int kernel, int dirs, hipStream_t st) {
  if (dirs < 1 || dirs > 3) return XCP_EINVAL;
  if (B <= 0 || T <= 0) return XCP_OK;
  if (H <= 0 || kernel < 0 || kernel > 1) return XCP_EINVAL;
#define XCP_LBD(VL, ST) lstm_bwd_dir_launch<VL, ST>(dout, dhn, dcn, whh, c0, cst, gates, dgates, dh0, dc0, work, lens, B, T, H, kernel, dirs, st)
  if (c0 || dh0 || dc0) return lens ? XCP_LBD(true, true) : XCP_LBD(false, true);
  return lens ? XCP_LBD(true, false) : XCP_LBD(false, false);
#undef XCP_LBD
}

}  // extern "C"

