// Class-activation maps (Grad-CAM / HiResCAM) of a backbone layer and their rendering.
// No reference op: build-defined.
//
// xcp_cam: per frame n and pixel p of an NHWC activation A [N][HW][CP] and its gradient G,
//   gradcam  (mode 0): raw[n][p] = sum_{c<C} w[n][c] * act(A[n][p][c]),  w = alpha if given, else
//                      w[n][c] = (sum_p G[n][p][c]) / HW  (p ascending per wave, waves ascending, one division)
//   hirescam (mode 1): raw[n][p] = sum_{c<C} G[n][p][c] * act(A[n][p][c])
//   act(a) = max(fmaf(a, scale[c], shift[c]), 0) when scale / shift are given (the exit map: conv4's raw
//   output under BN4 + ReLU, as avgpool_fwd_kernel forms it), otherwise a.
// One workgroup of 16 waves per frame.  A wave owns the pixels p = wave, wave + 16, ...; its 64 lanes own
// 8 consecutive channels each (one 16-byte load in bf16, two in fp32) of a 512-channel chunk and walk the
// chunks in ascending order, so every byte of A and G is read once, 1 KiB (2 KiB) contiguous per wave load.
// A pixel's sum: fp32 fmaf chain per lane (chunks ascending, channels ascending), then the xor-shuffle
// tree of wave_sum; lane 0 stores it.  The computed weights: per-lane fp32 sums over the wave's pixels, the
// 16 waves' partials through LDS summed in wave order.  No atomics: a run is reproducible bit for bit.
// Channels c >= C (the 728 flow's 8 pad channels) are loaded with their 16-byte group and discarded by a
// select, whatever they hold.  Per-channel vectors (alpha row, scale, shift) are staged in LDS once per
// frame, zero beyond C.  LDS: 16 x 512 floats of partials + 3 x 2048 floats = 56 KiB, hence C <= 2048.
//
// xcp_cam_render: raw [B*T][h][w] -> out [B*T][OH][OW]: r = max(raw, 0); normalize: r / max_p r at the
// low resolution (one IEEE division per map pixel; a map without a positive value stays zero), then
// bilinear up-sampling, align_corners=False, ATen's fp32 source-index and weight formulas (lin_idx, as
// frames.hip restates them for xcp_resize_bilinear), products then sums, no contraction.  Normalising
// before the interpolation keeps every output in [0, 1]: with a, b <= 1, fl(a l0) <= l0, fl(b l1) <= l1
// and fl(l0 + l1) = 1 for l0 = fl(1 - l1).  Frames t >= len[b] are zero.  A workgroup stages the whole
// map (h * w <= 8192 floats) and the output columns' indices and weights (OW <= 2048) in LDS and writes a
// band of whole output rows, lanes along the row; every band of a frame finds the same maximum (max is
// order-independent).
#include "common.h"

namespace {

constexpr int CAM_WAVES = 16;
constexpr int CAM_THREADS = CAM_WAVES * 64;
constexpr int CAM_CHUNK = 512;     // channels per wave load: 64 lanes x 8
constexpr int CAM_MAXC = 2048;
constexpr int RENDER_MAX_HW = 8192;
constexpr int RENDER_MAX_OW = 2048;

XCP_DEV float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// MODE 0: weights from LDS (alpha given or computed); MODE 1: weights are G at the pixel
template <typename T, int MODE, bool BN, bool MEAN>
__global__ __launch_bounds__(CAM_THREADS) void cam_kernel(const T* __restrict__ A, const float* __restrict__ a_scale,
                                                          const float* __restrict__ a_shift, const T* __restrict__ G,
                                                          const float* __restrict__ alpha, float* __restrict__ raw,
                                                          int HW, int C, int CP) {
  __shared__ __attribute__((aligned(16))) float part[CAM_WAVES][CAM_CHUNK];
  __shared__ __attribute__((aligned(16))) float sw[CAM_MAXC], ss[CAM_MAXC], st[CAM_MAXC];
  const int n = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nch = (C + CAM_CHUNK - 1) / CAM_CHUNK;
  const long frame = (long)n * HW * CP;

  if (BN || (MODE == 0 && !MEAN)) {
    for (int c = tid; c < nch * CAM_CHUNK; c += CAM_THREADS) {
      const bool in = c < C;
      if (BN) {
        ss[c] = in ? a_scale[c] : 0.f;
        st[c] = in ? a_shift[c] : 0.f;
      }
      if (MODE == 0 && !MEAN) sw[c] = in ? alpha[(long)n * C + c] : 0.f;
    }
  }
  if (MODE == 0 && MEAN) {
    // w[c] = mean_p G[p][c]: one chunk at a time, the waves' partial sums through LDS in wave order
    const float fhw = (float)HW;
    for (int ch = 0; ch < nch; ++ch) {
      const int c0 = ch * CAM_CHUNK + lane * 8;
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      if (c0 < C) {
#pragma unroll 4
        for (int p = wave; p < HW; p += CAM_WAVES) {
          float g[8];
          VecIO<T, 8>::load(G + frame + (long)p * CP + c0, g);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += g[j];
        }
      }
      VecIO<float, 8>::store(&part[wave][lane * 8], acc);
      __syncthreads();
      if (tid < CAM_CHUNK) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < CAM_WAVES; ++w) s += part[w][tid];
        const int c = ch * CAM_CHUNK + tid;
        sw[c] = c < C ? s / fhw : 0.f;
      }
      __syncthreads();
    }
  } else {
    __syncthreads();
  }

  for (int p = wave; p < HW; p += CAM_WAVES) {
    const T* ap = A + frame + (long)p * CP;
    float acc = 0.f;
#pragma unroll 2
    for (int ch = 0; ch < nch; ++ch) {
      const int c0 = ch * CAM_CHUNK + lane * 8;
      if (c0 < C) {   // c0 + 8 <= CP: C <= CP and CP % 8 == 0
        float a[8], w[8];
        VecIO<T, 8>::load(ap + c0, a);
        if (MODE == 1) VecIO<T, 8>::load(G + frame + (long)p * CP + c0, w);
        else VecIO<float, 8>::load(&sw[c0], w);
        if (BN) {
          float s[8], t[8];
          VecIO<float, 8>::load(&ss[c0], s);
          VecIO<float, 8>::load(&st[c0], t);
#pragma unroll
          for (int j = 0; j < 8; ++j) a[j] = fmaxf(fmaf(a[j], s[j], t[j]), 0.f);
        }
        const int nv = C - c0;   // channels of this group below C (8 or more: all)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = j < nv ? fmaf(w[j], a[j], acc) : acc;
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) raw[(long)n * HW + p] = acc;
  }
}

template <typename T, int MODE, bool BN>
int cam_launch2(const void* A, const float* s, const float* t, const void* G, const float* alpha, float* raw, int N,
                int HW, int C, int CP, hipStream_t st) {
  if (MODE == 0 && !alpha)
    hipLaunchKernelGGL((cam_kernel<T, MODE, BN, true>), dim3(N), dim3(CAM_THREADS), 0, st, (const T*)A, s, t, (const T*)G,
                       alpha, raw, HW, C, CP);
  else
    hipLaunchKernelGGL((cam_kernel<T, MODE, BN, false>), dim3(N), dim3(CAM_THREADS), 0, st, (const T*)A, s, t, (const T*)G,
                       alpha, raw, HW, C, CP);
  return (int)hipGetLastError();
}

template <typename T>
int cam_launch(int mode, const void* A, const float* s, const float* t, const void* G, const float* alpha, float* raw,
               int N, int HW, int C, int CP, hipStream_t st) {
  if (mode == 0) return s ? cam_launch2<T, 0, true>(A, s, t, G, alpha, raw, N, HW, C, CP, st)
                          : cam_launch2<T, 0, false>(A, s, t, G, alpha, raw, N, HW, C, CP, st);
  return s ? cam_launch2<T, 1, true>(A, s, t, G, alpha, raw, N, HW, C, CP, st)
           : cam_launch2<T, 1, false>(A, s, t, G, alpha, raw, N, HW, C, CP, st);
}

// ATen's upsample_bilinear2d source index and weights in fp32 (frames.hip lin_idx, restated)
XCP_DEV void cam_lin_idx(int dst, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = min((int)floorf(src), in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  float l = src - (float)i0;
  l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
  l1 = l;
  l0 = 1.f - l;
}

__global__ __launch_bounds__(256) void cam_render_kernel(const float* __restrict__ raw, const int* __restrict__ len,
                                                         float* __restrict__ out, int T, int h, int w, int OH, int OW,
                                                         float sh, float sw, int normalize, int bands, int rows) {
#pragma clang fp contract(off)
  extern __shared__ float r[];   // [h * w] the map, then the columns' tables [OW] x (w0, w1, lw0, lw1)
  __shared__ float red[4];
  const int f = blockIdx.x / bands, k = blockIdx.x - f * bands;
  const int tid = threadIdx.x;
  const int hw = h * w;
  const int r0 = k * rows, r1 = min(r0 + rows, OH);
  float* dst = out + (long)f * OH * OW;
  if (len != nullptr && f % T >= len[f / T]) {   // (uniform over the workgroup)
    for (int o = r0 * OW + tid; o < r1 * OW; o += 256) dst[o] = 0.f;
    return;
  }
  int* cw0 = reinterpret_cast<int*>(r + hw);
  int* cw1 = cw0 + OW;
  float* cl0 = reinterpret_cast<float*>(cw1 + OW);
  float* cl1 = cl0 + OW;
  for (int ow = tid; ow < OW; ow += 256) {
    int w0, w1;
    float lw0, lw1;
    cam_lin_idx(ow, w, sw, w0, w1, lw0, lw1);
    cw0[ow] = w0;
    cw1[ow] = w1;
    cl0[ow] = lw0;
    cl1[ow] = lw1;
  }
  const float* src = raw + (long)f * hw;
  float m = 0.f;
  for (int i = tid; i < hw; i += 256) {
    const float v = fmaxf(src[i], 0.f);
    r[i] = v;
    m = fmaxf(m, v);
  }
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  if (normalize && m > 0.f)
    for (int i = tid; i < hw; i += 256) r[i] = r[i] / m;   // (the elements this thread wrote)
  __syncthreads();
  for (int oh = r0; oh < r1; ++oh) {
    int h0, h1;
    float lh0, lh1;
    cam_lin_idx(oh, h, sh, h0, h1, lh0, lh1);
    const float* top = r + h0 * w;
    const float* bot = r + h1 * w;
    for (int ow = tid; ow < OW; ow += 256) {
      const int w0 = cw0[ow], w1 = cw1[ow];
      const float lw0 = cl0[ow], lw1 = cl1[ow];
      const float t0 = top[w0] * lw0 + top[w1] * lw1;
      const float t1 = bot[w0] * lw0 + bot[w1] * lw1;
      dst[(long)oh * OW + ow] = t0 * lh0 + t1 * lh1;
    }
  }
}

}  // namespace

extern "C" {

int xcp_cam(int dtype, int mode, const void* A, const float* a_scale, const float* a_shift, const void* G,
            const float* alpha, float* raw, int N, int HW, int C, int CP, hipStream_t stream) {
  if (!A || !raw || N <= 0 || HW <= 0 || C <= 0 || CP <= 0) return XCP_EINVAL;
  if (C > CP || CP % 8) return XCP_EINVAL;
  if ((a_scale == nullptr) != (a_shift == nullptr)) return XCP_EINVAL;
  if (mode == 0 ? (!G && !alpha) : (mode != 1 || !G || alpha)) return XCP_EINVAL;
  if (dtype != XCP_F32 && dtype != XCP_BF16) return XCP_EUNSUPPORTED;
  if (C > CAM_MAXC) return XCP_EUNSUPPORTED;   // the per-channel vectors' LDS
  if (dtype == XCP_BF16) return cam_launch<bf16>(mode, A, a_scale, a_shift, G, alpha, raw, N, HW, C, CP, stream);
  return cam_launch<float>(mode, A, a_scale, a_shift, G, alpha, raw, N, HW, C, CP, stream);
}

int xcp_cam_render(const float* raw, const int* len, float* out, int B, int T, int h, int w, int OH, int OW,
                   int normalize, hipStream_t stream) {
  if (!raw || !out || B <= 0 || T <= 0 || h <= 0 || w <= 0 || OH <= 0 || OW <= 0) return XCP_EINVAL;
  if (normalize != 0 && normalize != 1) return XCP_EINVAL;
  if ((long)h * w > RENDER_MAX_HW || OW > RENDER_MAX_OW) return XCP_EUNSUPPORTED;   // the map's, the columns' LDS
  // a workgroup writes a band of whole output rows, about 8192 outputs
  const int rows = OW >= 8192 ? 1 : (8192 / OW < OH ? 8192 / OW : OH);
  const long bands = (OH + rows - 1) / rows;
  if ((long)B * T * bands > 0x7fffffffL) return XCP_EUNSUPPORTED;
  hipLaunchKernelGGL(cam_render_kernel, dim3((unsigned)((long)B * T * bands)), dim3(256),
                     ((size_t)h * w + 4 * (size_t)OW) * sizeof(float), stream, raw, len, out, T, h, w, OH, OW,
                     (float)h / (float)OH, (float)w / (float)OW, normalize, (int)bands, rows);
  return (int)hipGetLastError();
}

}  // extern "C"
