// Clip input conversion on the GPU: uint8 face frames -> the model's fp32 input.
//
// Reference: FaceDataset.__getitem__ (video_dataloader.py:22-37) turns an .npy clip of
// uint8 [T, H, W, 3] into fp32 [T, 3, H, W] / 255 (no mean / std), and collate_fn
// (video_dataloader.py:53-68) zero-pads T to the batch maximum.  Done on the host that is
// 4 bytes per subpixel over PCIe; here the host ships the uint8 clips (a quarter of the
// bytes) and this kernel expands them in HBM, bit-identical to the host path (the same
// IEEE single-precision x / 255).
//
// in  [B][Tmax][H][W][3] uint8 (frames t >= len[b] are ignored, their output is zero)
// out [B][Tmax][3][H][W] fp32
// One thread converts 4 consecutive pixels of one row: one 12-byte read, three 16-byte
// stores (one per channel plane).  HBM-bound: 3 + 12 bytes per pixel.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void frames_u8_kernel(const unsigned char* __restrict__ in,
                                                        const int* __restrict__ len, float* __restrict__ out, int Tmax,
                                                        int H, int W, long total) {
  const int W4 = W / 4;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const long per_frame = (long)H * W4;
  const long frame = g / per_frame;               // b * Tmax + t
  const long r = g - frame * per_frame;
  const int h = (int)(r / W4), w0 = (int)(r - (long)h * W4) * 4;
  const int b = (int)(frame / Tmax), t = (int)(frame - (long)b * Tmax);
  float v[3][4];
  if (t < len[b]) {
    const unsigned* src = reinterpret_cast<const unsigned*>(in + ((frame * H + h) * W + w0) * 3);
    const unsigned u[3] = {src[0], src[1], src[2]};   // 12 bytes: pixels w0..w0+3, RGB interleaved
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const unsigned byte = (u[k >> 2] >> (8 * (k & 3))) & 0xffu;
      v[k % 3][k / 3] = (float)byte / 255.f;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int p = 0; p < 4; ++p) v[c][p] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    *reinterpret_cast<float4*>(out + (((frame * 3 + c) * H + h) * W + w0)) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
}


// Bilinear resize, align_corners=False (F.interpolate(..., mode="bilinear"), as the audio
// front end XceptionLSTMA.py:46 uses it: MFCC [B*T, 3, 13, 1] -> [B*T, 3, 64, 64]).
// Source coordinates, indices and weights follow ATen's upsample_bilinear2d in fp32:
//   src = max(scale * (dst + 0.5) - 0.5, 0), scale = in / out, i0 = min(floor(src), in - 1),
//   i1 = i0 + (i0 < in - 1), l1 = clamp(src - i0, 0, 1), l0 = 1 - l1,
//   out = (a * w0 + b * w1) * h0 + (c * w0 + d * w1) * h1  (products, then sums).
// in [NC][IH][IW], out [NC][OH][OW] fp32; one thread per output pixel.
XCP_DEV void lin_idx(int dst, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
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

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                              int IH, int IW, int OH, int OW, float sh, float sw,
                                                              long total) {
#pragma clang fp contract(off)
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const long plane = g / ((long)OH * OW);
  const int r = (int)(g - plane * OH * OW), oh = r / OW, ow = r - oh * OW;
  int h0, h1, w0, w1;
  float lh0, lh1, lw0, lw1;
  lin_idx(oh, IH, sh, h0, h1, lh0, lh1);
  lin_idx(ow, IW, sw, w0, w1, lw0, lw1);
  const float* p = in + plane * IH * IW;
  const float t0 = p[h0 * IW + w0] * lw0 + p[h0 * IW + w1] * lw1;
  const float t1 = p[h1 * IW + w0] * lw0 + p[h1 * IW + w1] * lw1;
  out[g] = t0 * lh0 + t1 * lh1;
}

// General clip preparation: uint8 frames -> x / 255, optionally bilinear-resized to OH x OW
// (F.interpolate(x / 255, (OH, OW), mode="bilinear", align_corners=False) of the fp32 clip, as
// lin_idx above), stored fp32 or bf16 (round to nearest even of that fp32 value), planar
// [B][Tmax][3][OH][OW] or interleaved [B][Tmax][OH][OW][3].  One thread per output pixel
// (3 channels); frames past a clip's length are zero.
template <typename T, bool NHWC>
__global__ __launch_bounds__(256) void frames_prep_kernel(const unsigned char* __restrict__ in,
                                                          const int* __restrict__ len, T* __restrict__ out, int Tmax,
                                                          int H, int W, int OH, int OW, float sh, float sw, long total) {
#pragma clang fp contract(off)
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const long per_frame = (long)OH * OW;
  const long frame = g / per_frame;
  const int r = (int)(g - frame * per_frame), oh = r / OW, ow = r - oh * OW;
  const int b = (int)(frame / Tmax), t = (int)(frame - (long)b * Tmax);
  float v[3] = {0.f, 0.f, 0.f};
  if (t < len[b]) {
    const unsigned char* f = in + frame * H * W * 3;
    if (OH == H && OW == W) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (float)f[((long)oh * W + ow) * 3 + c] / 255.f;
    } else {
      int h0, h1, w0, w1;
      float lh0, lh1, lw0, lw1;
      lin_idx(oh, H, sh, h0, h1, lh0, lh1);
      lin_idx(ow, W, sw, w0, w1, lw0, lw1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = (float)f[((long)h0 * W + w0) * 3 + c] / 255.f, bb = (float)f[((long)h0 * W + w1) * 3 + c] / 255.f;
        const float cc = (float)f[((long)h1 * W + w0) * 3 + c] / 255.f, d = (float)f[((long)h1 * W + w1) * 3 + c] / 255.f;
        const float t0 = a * lw0 + bb * lw1;
        const float t1 = cc * lw0 + d * lw1;
        v[c] = t0 * lh0 + t1 * lh1;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long o = NHWC ? g * 3 + c : ((frame * 3 + c) * OH + oh) * OW + ow;
    out[o] = (T)v[c];
  }
}

template <typename T>
void launch_prep(const unsigned char* in, const int* len, void* out, bool nhwc, int Tmax, int H, int W, int OH, int OW,
                 long total, hipStream_t st) {
  const dim3 grid((unsigned)((total + 255) / 256));
  const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
  if (nhwc)
    hipLaunchKernelGGL((frames_prep_kernel<T, true>), grid, dim3(256), 0, st, in, len, (T*)out, Tmax, H, W, OH, OW, sh,
                       sw, total);
  else
    hipLaunchKernelGGL((frames_prep_kernel<T, false>), grid, dim3(256), 0, st, in, len, (T*)out, Tmax, H, W, OH, OW, sh,
                       sw, total);
}

// Clip augmentation: the same uint8 clips -> the model's input with a per-clip random crop box
// resampled to OH x OW, horizontal flip, per-channel affine (contrast / brightness / mean / std),
// erase rectangle and frame sub-sampling, one read of the clip and one write of the input.
// tab [B][XCP_AUG_COLS] int32 (device), one row per clip, every frame of the clip uses it:
//   0 t0, 1 tstride, 2 y0, 3 x0, 4 bh, 5 bw, 6 flip, 7 ey0, 8 ex0, 9 eh, 10 ew, 11 unused,
//   12-14 a[3], 15-17 b[3], 18-20 fill[3] (fp32 bit patterns), 21-23 unused.
// Order of operations (the contract augment_reference restates): x / 255; bilinear resample of
// the box (lin_idx on box-relative indices, products then sums as frames_prep_kernel); flip;
// v * a[c], then + b[c] (two roundings, no FMA); fill inside the erase rectangle; cast.
//
// A 256-thread block makes a 16-row x 128-column tile of one output frame: wave w the rows
// 4w..4w+3, lane l the columns l and l + 64.  A thread forms its 2 column and 4 row index /
// weight sets once (the row sets and all row addressing in scalar registers), fetches each
// source pixel pair (i1 is i0 or i0 + 1: 6 consecutive bytes) with one 8-byte load, all 16 loads
// ahead of the arithmetic, and computes its two pixels of a row as the halves of packed fp32
// instructions.  Planar stores are one element per lane along a row; interleaved stores go
// through three ds_permute so that lane j holds element j, j + 64, j + 128 of the wave's 192
// contiguous elements.  No LDS.
constexpr int AUG_COLS = 24, AUG_TR = 16, AUG_TC = 128;

template <bool V> struct AugBool { static constexpr bool value = V; };

struct AugClip {   // one clip's table row, clamped into the valid range
  int t0, ts, y0, x0, bh, bw, flip, ey_lo, ey_hi, ex_lo, ex_hi, out_len;
};

XCP_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

XCP_DEV AugClip aug_clip(const int* __restrict__ r, int len, int Tmax, int Tout, int H, int W, int OH, int OW) {
  AugClip p;
  const int L = clampi(len, 0, Tmax);
  p.t0 = clampi(r[0], 0, Tmax);
  p.ts = clampi(r[1], 1, Tmax);
  p.bh = clampi(r[4], 1, H);
  p.bw = clampi(r[5], 1, W);
  p.y0 = clampi(r[2], 0, H - p.bh);
  p.x0 = clampi(r[3], 0, W - p.bw);
  p.flip = r[6] != 0;
  const long ey1 = (long)r[7] + r[9], ex1 = (long)r[8] + r[10];   // eh, ew <= 0: empty
  p.ey_lo = max(r[7], 0);
  p.ey_hi = (int)(ey1 < (long)OH ? ey1 : (long)OH);
  p.ex_lo = max(r[8], 0);
  p.ex_hi = (int)(ex1 < (long)OW ? ex1 : (long)OW);
  const int n = L > p.t0 ? (L - p.t0 + p.ts - 1) / p.ts : 0;
  p.out_len = n < Tout ? n : Tout;
  return p;
}

// (float)byte / 255.f, correctly rounded, without the division sequence: 1 / 255 as the
// unevaluated sum of two floats, x * hi + fl(x * lo) in one fma.  Exact for every x in 0..255
// (all 256 checked against x / 255.f on the host; the GPU tests feed every byte value).
XCP_DEV f32x2 u8_unit(f32x2 x) {
  const float hi = 0x1.010102p-8f, lo = -0x1.fdfdfep-33f;
  const f32x2 l = x * lo;
  return __builtin_elementwise_fma(x, f32x2{hi, hi}, l);
}

// channel c of the pixels p0 and p1 (3 bytes each) as floats 0..255
XCP_DEV f32x2 px2(unsigned p0, unsigned p1, int c) {
  return f32x2{(float)((p0 >> (8 * c)) & 0xffu), (float)((p1 >> (8 * c)) & 0xffu)};
}

// The 3 bytes of the source pixel at byte offset off of in (-> p0, byte c = channel c) and of its
// right neighbour, or of itself again when same (-> p1): lin_idx gives i1 = i0 or i0 + 1, so the
// two are 6 consecutive bytes and one 8-byte load brings both.  last8 = (bytes of in) - 8 keeps
// that load inside the buffer: at the buffer's end it starts s <= 2 (a single pixel: s <= 5)
// bytes early and the wanted bytes are shifted down.  A buffer under 8 bytes is read bytewise.
// load_px_pair issues the load, split_px_pair (given the same cw, lim, same) takes the bytes
// apart, so that a thread can issue all its loads before it waits for the first.  The pixel is at
// byte row + cw of in (row: wave-uniform, cw: per lane); lim = last8 - row, clamped to an int.
template <bool WIDE>
XCP_DEV unsigned long long load_px_pair(const unsigned char* __restrict__ in, long row, int cw, int lim, bool same) {
  unsigned long long u;
  if (WIDE) {
    __builtin_memcpy(&u, in + row + min(cw, lim), 8);
  } else {
    const unsigned char* s = in + row + cw;
    const int o1 = same ? 0 : 3;
    const unsigned p0 = (unsigned)s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16;
    const unsigned p1 = (unsigned)s[o1] | (unsigned)s[o1 + 1] << 8 | (unsigned)s[o1 + 2] << 16;
    u = (unsigned long long)p0 | (unsigned long long)p1 << 24;
  }
  return u;
}

template <bool WIDE>
XCP_DEV void split_px_pair(unsigned long long u, int cw, int lim, bool same, unsigned& p0, unsigned& p1) {
  if (WIDE) u >>= 8 * (cw - min(cw, lim));
  p0 = (unsigned)u & 0xffffffu;
  p1 = same ? p0 : (unsigned)(u >> 24) & 0xffffffu;
}

// One wave stores the 3 channels v of 64 pixels (lane l: column c0 + l) of output row oh; ok
// (wave-uniform) = the row and c0 are inside the frame.  Every lane of the wave calls it.
template <typename T, bool NHWC>
XCP_DEV void aug_store(T* __restrict__ out, const float* v, int frame, int oh, int c0, int lane, int OH, int OW,
                       bool ok) {
  if (NHWC) {
    // lane l sends channel c to lane (3l + c) mod 64 (3 is invertible mod 64: no collision);
    // element e = lane + 64k of the wave's 192 is channel e % 3 = (lane + k) % 3 of pixel e / 3
    float rc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      rc[c] = __int_as_float(__builtin_amdgcn_ds_permute(((3 * lane + c) & 63) * 4, __float_as_int(v[c])));
    const int nel = ok ? 3 * min(64, OW - c0) : 0, m = lane % 3;
    T* o = out + (((long)frame * OH + oh) * OW + c0) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int cs = m + k >= 3 ? m + k - 3 : m + k;
      const float x = cs == 0 ? rc[0] : (cs == 1 ? rc[1] : rc[2]);
      if (lane + 64 * k < nel) o[lane + 64 * k] = (T)x;
    }
  } else if (ok && c0 + lane < OW) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(((long)frame * 3 + c) * OH + oh) * OW + c0 + lane] = (T)v[c];
  }
}

template <typename T, bool NHWC>
__global__ __launch_bounds__(256) void clip_augment_kernel(const unsigned char* __restrict__ in,
                                                           const int* __restrict__ len, const int* __restrict__ tab,
                                                           T* __restrict__ out, int* __restrict__ out_len, int Tmax,
                                                           int Tout, int H, int W, int OH, int OW, int tiles_y,
                                                           int tiles_x, long last8) {
#pragma clang fp contract(off)
  const int per_frame = tiles_y * tiles_x;
  const int frame = blockIdx.x / per_frame;   // b * Tout + t
  const int tile = blockIdx.x - frame * per_frame, ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int b = frame / Tout, t = frame - b * Tout;
  const int* row = tab + (long)b * AUG_COLS;
  const AugClip p = aug_clip(row, len[b], Tmax, Tout, H, W, OH, OW);
  if (t == 0 && tile == 0 && threadIdx.x == 0) out_len[b] = p.out_len;
  const bool live = t < p.out_len;   // block-uniform
  // the wave index and what follows from it (rows, source rows, store bases) in scalar registers
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int oh0 = ty * AUG_TR + wave * 4, ow0 = tx * AUG_TC;

  float av[3], bv[3], fv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    av[c] = __int_as_float(row[12 + c]);
    bv[c] = __int_as_float(row[15 + c]);
    fv[c] = __int_as_float(row[18 + c]);
  }
  // per-column sets: byte offsets of the two source columns inside a source row, weights, erase
  int cw0[2];
  float clw0[2], clw1[2];
  bool cer[2], csame[2];
  const float sh = (float)p.bh / (float)OH, sw = (float)p.bw / (float)OW;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ow = min(ow0 + j * 64 + lane, OW - 1);   // lanes past the row work on its last column, unstored
    int w0, w1;
    lin_idx(p.flip ? OW - 1 - ow : ow, p.bw, sw, w0, w1, clw0[j], clw1[j]);
    cw0[j] = (p.x0 + w0) * 3;
    csame[j] = w1 == w0;
    cer[j] = ow >= p.ex_lo && ow < p.ex_hi;
  }
  if (!live) {   // padding frame: zeros, nothing read
    const float z[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        aug_store<T, NHWC>(out, z, frame, oh0 + i, ow0 + j * 64, lane, OH, OW, oh0 + i < OH && ow0 + j * 64 < OW);
    return;
  }
  const long f = ((long)b * Tmax + p.t0 + t * p.ts) * H * W * 3;   // byte offset of the source frame
  // Rows past OH recompute row OH - 1 and store nothing.  The thread's 16 loads (4 rows x 2
  // columns x 2 source rows) are issued before the first is used.
  auto rows = [&](auto wide) {
#pragma clang fp contract(off)
  constexpr bool WIDE = decltype(wide)::value;
  const f32x2 lw0 = {clw0[0], clw0[1]}, lw1 = {clw1[0], clw1[1]};
  int lim[4][2];
  float lh[4][2];
  unsigned long long u[4][2][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int h[2];
    lin_idx(min(oh0 + i, OH - 1), p.bh, sh, h[0], h[1], lh[i][0], lh[i][1]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const long r = f + (long)(p.y0 + __builtin_amdgcn_readfirstlane(h[k])) * W * 3;
      const long d = last8 - r;
      lim[i][k] = (int)(d > 0x7fffffffL ? 0x7fffffffL : (d < -0x7fffffffL ? -0x7fffffffL : d));
#pragma unroll
      for (int j = 0; j < 2; ++j) u[i][j][k] = load_px_pair<WIDE>(in, r, cw0[j], lim[i][k], csame[j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int oh = oh0 + i, ohc = min(oh, OH - 1);
    const float lh0 = lh[i][0], lh1 = lh[i][1];
    const bool rer = ohc >= p.ey_lo && ohc < p.ey_hi;
    unsigned q[2][2][2];   // [column set][source row][source column]: a pixel's 3 bytes
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 2; ++k)
        split_px_pair<WIDE>(u[i][j][k], cw0[j], lim[i][k], csame[j], q[j][k][0], q[j][k][1]);
    // the thread's two pixels of the row side by side in the halves of f32x2 values: the same
    // IEEE operations per pixel, in half as many (packed) instructions
    float v[2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x2 a = u8_unit(px2(q[0][0][0], q[1][0][0], c)), bb = u8_unit(px2(q[0][0][1], q[1][0][1], c));
      const f32x2 cc = u8_unit(px2(q[0][1][0], q[1][1][0], c)), d = u8_unit(px2(q[0][1][1], q[1][1][1], c));
      const f32x2 t0 = a * lw0 + bb * lw1;
      const f32x2 t1 = cc * lw0 + d * lw1;
      f32x2 x = t0 * lh0 + t1 * lh1;
      x = x * av[c];
      x = x + bv[c];
      v[0][c] = (rer && cer[0]) ? fv[c] : x.x;
      v[1][c] = (rer && cer[1]) ? fv[c] : x.y;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
      aug_store<T, NHWC>(out, v[j], frame, oh, ow0 + j * 64, lane, OH, OW, oh < OH && ow0 + j * 64 < OW);
  }
  };
  if (last8 >= 0)   // grid-uniform
    rows(AugBool<true>{});
  else
    rows(AugBool<false>{});
}

template <typename T>
void launch_augment(const unsigned char* in, const int* len, const int* tab, void* out, int* out_len, bool nhwc,
                    int Tmax, int Tout, int H, int W, int OH, int OW, int tiles_y, int tiles_x, long last8,
                    unsigned blocks, hipStream_t st) {
  if (nhwc)
    hipLaunchKernelGGL((clip_augment_kernel<T, true>), dim3(blocks), dim3(256), 0, st, in, len, tab, (T*)out, out_len,
                       Tmax, Tout, H, W, OH, OW, tiles_y, tiles_x, last8);
  else
    hipLaunchKernelGGL((clip_augment_kernel<T, false>), dim3(blocks), dim3(256), 0, st, in, len, tab, (T*)out, out_len,
                       Tmax, Tout, H, W, OH, OW, tiles_y, tiles_x, last8);
}

}  // namespace

extern "C" {

// Clip augmentation (layout of tab, order of operations: clip_augment_kernel above).  in
// [B][Tmax][H][W][3] uint8, len [B], tab [B][24] int32 -> out [B][Tout][3][OH][OW] (nhwc 1:
// [B][Tout][OH][OW][3]) of dtype, out_len [B] int32; all device, stream-ordered, no host read.
int xcp_clip_augment(const unsigned char* in, const int* len, const int* tab, void* out, int* out_len, int B, int Tmax,
                     int Tout, int H, int W, int OH, int OW, int dtype, int nhwc, hipStream_t st) {
  if (B <= 0 || Tout <= 0 || OH <= 0 || OW <= 0) return XCP_OK;
  if (Tmax <= 0 || H <= 0 || W <= 0 || (dtype != XCP_F32 && dtype != XCP_BF16)) return XCP_EINVAL;
  const int tiles_y = (OH + AUG_TR - 1) / AUG_TR, tiles_x = (OW + AUG_TC - 1) / AUG_TC;
  const long blocks = (long)B * Tout * tiles_y * tiles_x;
  if (blocks > 0x7fffffffL) return XCP_EUNSUPPORTED;
  const long last8 = (long)B * Tmax * H * W * 3 - 8;   // where the last 8-byte load inside in starts
  if (dtype == XCP_F32)
    launch_augment<float>(in, len, tab, out, out_len, nhwc != 0, Tmax, Tout, H, W, OH, OW, tiles_y, tiles_x, last8,
                          (unsigned)blocks, st);
  else
    launch_augment<bf16>(in, len, tab, out, out_len, nhwc != 0, Tmax, Tout, H, W, OH, OW, tiles_y, tiles_x, last8,
                         (unsigned)blocks, st);
  return (int)hipGetLastError();
}

// B clips of up to Tmax uint8 [H][W][3] frames (len: device int32 [B]) -> out at OH x OW:
// dtype XCP_F32 / XCP_BF16, nhwc 0 = [B][Tmax][3][OH][OW], 1 = [B][Tmax][OH][OW][3]
int xcp_frames_prep(const unsigned char* in, const int* len, void* out, int B, int Tmax, int H, int W, int OH, int OW,
                    int dtype, int nhwc, hipStream_t st) {
  if (B <= 0 || Tmax <= 0 || OH <= 0 || OW <= 0) return XCP_OK;
  if (H <= 0 || W <= 0 || (dtype != XCP_F32 && dtype != XCP_BF16)) return XCP_EINVAL;
  const long total = (long)B * Tmax * OH * OW;
  if (dtype == XCP_F32)
    launch_prep<float>(in, len, out, nhwc != 0, Tmax, H, W, OH, OW, total, st);
  else
    launch_prep<bf16>(in, len, out, nhwc != 0, Tmax, H, W, OH, OW, total, st);
  return (int)hipGetLastError();
}

// B clips of up to Tmax frames (len: device int32 [B]); W must be a multiple of 4
int xcp_frames_u8_to_f32(const unsigned char* in, const int* len, float* out, int B, int Tmax, int H, int W,
                         hipStream_t st) {
  if (B <= 0 || Tmax <= 0 || H <= 0 || W <= 0) return XCP_OK;
  if (W % 4) return XCP_EINVAL;
  const long total = (long)B * Tmax * H * (W / 4);
  hipLaunchKernelGGL(frames_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, len, out, Tmax, H,
                     W, total);
  return (int)hipGetLastError();
}

// out [NC][OH][OW] = bilinear resize (align_corners=False) of in [NC][IH][IW], fp32
int xcp_resize_bilinear(const float* in, float* out, int NC, int IH, int IW, int OH, int OW, hipStream_t st) {
  if (NC <= 0 || OH <= 0 || OW <= 0) return XCP_OK;
  if (IH <= 0 || IW <= 0) return XCP_EINVAL;
  const long total = (long)NC * OH * OW;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, out, IH, IW,
                     OH, OW, (float)IH / (float)OH, (float)IW / (float)OW, total);
  return (int)hipGetLastError();
}

}  // extern "C"
