// Clip degradation: Gaussian blur, sensor noise and baseline 4:2:0 JPEG of the uint8 clip, one launch,
// one read of the clip and one write (xcp/degrade.py states the integer arithmetic and restates it in
// numpy; the two agree byte for byte).
//
// One 256-thread workgroup makes a 32 x 32 tile (2 x 2 macroblocks) of one frame, wholly in LDS:
//   region  the pixels whose blurred + noised value the tile needs: the tile itself, or with JPEG the tile
//           and a ring of 16 pixels (64 x 64, 4 x 4 macroblocks) -- the triangle chroma up-sampling reads one
//           chroma sample across the tile border, and that sample is only known once its whole 8 x 8 chroma
//           block (16 x 16 pixels) went through the DCT and the quantiser, so the ring's chroma blocks are
//           recomputed here (luma only inside the tile: 16 luma + 2 x 16 chroma blocks);
//   input   the region and a halo of R pixels for the blur, indices reflected at the frame border.
// Region pixels outside the frame take the value of the nearest frame pixel (the edge-replicated padding
// to whole macroblocks); chroma blocks outside the padded plane are computed and never read.
#include "common.h"

namespace {

constexpr int DEG_COLS = 16;               // XCP_DEG_COLS
constexpr int TILE = 32, MARG = 16, RMAX = 7;
constexpr int REG = TILE + 2 * MARG;       // 64: region side with JPEG
constexpr int INW = REG + 2 * RMAX;        // 78: input side at most
constexpr int BLK = 72;                    // ints per 8 x 8 block in LDS: rows of 9 (row and column passes conflict-free)
constexpr int NBLK = 48;                   // 16 luma, 16 Cb, 16 Cr

constexpr int DC[8][8] = {{1448, 1448, 1448, 1448, 1448, 1448, 1448, 1448},
                          {2009, 1703, 1138, 400, -400, -1138, -1703, -2009},
                          {1892, 784, -784, -1892, -1892, -784, 784, 1892},
                          {1703, -400, -2009, -1138, 1138, 2009, 400, -1703},
                          {1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448},
                          {1138, -2009, 400, 1703, -1703, -400, 2009, -1138},
                          {784, -1892, 1892, -784, -784, 1892, -1892, 784},
                          {400, -1138, 1703, -2009, 2009, -1703, 1138, -400}};   // C[u][x]

__constant__ unsigned char QBASE[128] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99,
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

XCP_DEV int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
XCP_DEV int rs(int a, int n) { return (a + (1 << (n - 1))) >> n; }
// reflect-101, then clamped (frames smaller than the radius)
XCP_DEV int refl(int i, int n) { return clampi(i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i), 0, n - 1); }

// Philox4x32-10, counter (c0, c1, c2, 0), key (k0, k1) -> the sum of the eight 16-bit halves of its output
XCP_DEV int philox_halves(unsigned c0, unsigned c1, unsigned c2, unsigned k0, unsigned k1) {
  unsigned c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return (int)((c0 & 0xffffu) + (c0 >> 16) + (c1 & 0xffffu) + (c1 >> 16) + (c2 & 0xffffu) + (c2 >> 16) +
               (c3 & 0xffffu) + (c3 >> 16));
}

// out[u] = rs(sum_x C[u][x] in[x], SH)   (forward passes; TR: out[x] = rs(sum_u C[u][x] in[u], SH), inverse)
template <bool TR, int SH>
XCP_DEV void dct8(const int* in, int* out) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    int a = 0;
#pragma unroll
    for (int x = 0; x < 8; ++x) a += __mul24(TR ? DC[x][u] : DC[u][x], in[x]);   // |in| < 2^17: exact, full rate
    out[u] = rs(a, SH);
  }
}

__global__ __launch_bounds__(256) void clip_degrade_kernel(const unsigned char* __restrict__ in,
                                                           const int* __restrict__ len, const int* __restrict__ tab,
                                                           unsigned char* __restrict__ out, int Tmax, int H, int W,
                                                           int tiles_y, int tiles_x) {
  // s_a: the input (u8 [IW][IW][3], 18252 B) and the row-filtered plane (int [IW][RW], 19968 B); once the
  // region is made, the 48 DCT blocks (13824 B) lie over both
  __shared__ __attribute__((aligned(16))) unsigned char s_a[18256 + INW * REG * 4];
  __shared__ __attribute__((aligned(16))) unsigned char s_px[REG * REG * 3];   // the region, u8 [RW][RW][3]; then the tile's bytes [32][96]
  __shared__ int s_q[128];
  unsigned char* const s_in = s_a;
  int* const s_h = reinterpret_cast<int*>(s_a + 18256);
  int* const s_d = reinterpret_cast<int*>(s_a);

  const int tid = threadIdx.x;
  const int per_frame = tiles_y * tiles_x;
  const int frame = blockIdx.x / per_frame;   // b * Tmax + t
  const int tile = blockIdx.x - frame * per_frame, ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int b = frame / Tmax, t = frame - b * Tmax;
  const int* row = tab + (long)b * DEG_COLS;
  const int q = clampi(row[0], 0, 100), R = clampi(row[1], 0, RMAX), namp = clampi(row[10], 0, 1023);
  const bool live = t < clampi(len[b], 0, Tmax);   // block-uniform
  const long fbase = (long)frame * H * W * 3;      // byte offset of the frame, in and out
  const int ty0 = ty * TILE, tx0 = tx * TILE;

  if (!live) {
    for (int i = tid; i < TILE * TILE * 3 / 4; i += 256) reinterpret_cast<unsigned*>(s_px)[i] = 0u;
  } else {
    const int M = q > 0 ? MARG : 0, RW = TILE + 2 * M, sh = q > 0 ? 6 : 5, IW = RW + 2 * R;
    const int ry0 = ty0 - M, rx0 = tx0 - M;
    const unsigned char* src = in + fbase;
    {   // the input: frame pixel (refl(ry0 - R + i), refl(rx0 - R + j)) at [i][j]; without blur this is the region
        // itself, whose pixels outside the frame are the nearest frame pixel's
      unsigned char* dst = R > 0 ? s_in : s_px;
      for (int idx = tid; idx < IW * IW; idx += 256) {
        const int i = idx / IW, j = idx - i * IW;
        const int gy = R > 0 ? refl(ry0 - R + i, H) : clampi(ry0 + i, 0, H - 1);
        const int gx = R > 0 ? refl(rx0 - R + j, W) : clampi(rx0 + j, 0, W - 1);
        const unsigned char* p = src + ((long)gy * W + gx) * 3;
        dst[idx * 3] = p[0];
        dst[idx * 3 + 1] = p[1];
        dst[idx * 3 + 2] = p[2];
      }
    }
    __syncthreads();
    if (R > 0) {   // block-uniform
      // 24-bit multiplies (full rate): taps below 2^12 times sums below 2^21, exact for every table whose
      // passes sum to 2048; other taps are read as their low 24 bits
      int w[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) w[k] = k <= R ? row[2 + k] : 0;
      for (int c = 0; c < 3; ++c) {
        // rows: every input row at the region's (clamped) columns
        for (int idx = tid; idx < IW * RW; idx += 256) {
          const int i = idx >> sh, x = idx & (RW - 1);
          const int xc = clampi(clampi(rx0 + x, 0, W - 1) - rx0 + R, R, IW - 1 - R);   // column of the centre tap
          const unsigned char* p = s_in + (i * IW + xc) * 3 + c;
          int a = __mul24(w[0], p[0]);
#pragma unroll
          for (int k = 1; k <= RMAX; ++k)
            if (k <= R) a += __mul24(w[k], p[-3 * k] + p[3 * k]);
          s_h[idx] = a;
        }
        __syncthreads();
        // columns
        for (int idx = tid; idx < RW * RW; idx += 256) {
          const int y = idx >> sh, x = idx & (RW - 1);
          const int yc = clampi(clampi(ry0 + y, 0, H - 1) - ry0 + R, R, IW - 1 - R);
          const int* p = s_h + (yc << sh) + x;
          int a = __mul24(w[0], p[0]);
#pragma unroll
          for (int k = 1; k <= RMAX; ++k)
            if (k <= R) a += __mul24(w[k], p[-(k << sh)] + p[k << sh]);
          s_px[idx * 3 + c] = (unsigned char)clampi(rs(a, 22), 0, 255);
        }
        __syncthreads();
      }
    }
    if (namp > 0) {
      const unsigned k0 = (unsigned)row[11], k1 = (unsigned)row[12];
      for (int idx = tid; idx < RW * RW * 3; idx += 256) {
        const int pix = idx / 3, c = idx - pix * 3;
        const int y = pix >> sh, x = pix & (RW - 1);
        const int yc = clampi(ry0 + y, 0, H - 1), xc = clampi(rx0 + x, 0, W - 1);
        const int S = philox_halves((unsigned)yc * (unsigned)W + (unsigned)xc, (unsigned)t, (unsigned)c, k0, k1);
        const int n = rs(namp * (2 * S - 524280), 20);
        s_px[idx] = (unsigned char)clampi((int)s_px[idx] + n, 0, 255);
      }
      __syncthreads();
    }
    if (q > 0) {   // block-uniform; RW = 64, the tile at (16, 16) of the region
      if (tid < 128) {
        const int s = q < 50 ? 5000 / q : 200 - 2 * q;
        s_q[tid] = clampi(((int)QBASE[tid] * s + 50) / 100, 1, 255);
      }
      // colour conversion: luma of the tile, 2 x 2-averaged chroma of the region, level-shifted, in blocks
      for (int idx = tid; idx < TILE * TILE; idx += 256) {
        const int y = idx >> 5, x = idx & 31;
        const unsigned char* p = s_px + ((y + MARG) * REG + x + MARG) * 3;
        const int Y = (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16;
        s_d[((y >> 3) * 4 + (x >> 3)) * BLK + (y & 7) * 9 + (x & 7)] = Y - 128;
        int cb = 2, cr = 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned char* pc = s_px + ((2 * y + (e >> 1)) * REG + 2 * x + (e & 1)) * 3;
          cb += (-11059 * pc[0] - 21709 * pc[1] + 32768 * pc[2] + (128 << 16) + 32767) >> 16;
          cr += (32768 * pc[0] - 27439 * pc[1] - 5329 * pc[2] + (128 << 16) + 32767) >> 16;
        }
        const int o = ((y >> 3) * 4 + (x >> 3)) * BLK + (y & 7) * 9 + (x & 7);
        s_d[16 * BLK + o] = (cb >> 2) - 128;
        s_d[32 * BLK + o] = (cr >> 2) - 128;
      }
      __syncthreads();
      for (int id = tid; id < NBLK * 8; id += 256) {   // forward, along x: a thread per block row
        int* p = s_d + (id >> 3) * BLK + (id & 7) * 9;
        int a[8], o[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) a[x] = p[x];
        dct8<false, 9>(a, o);
#pragma unroll
        for (int x = 0; x < 8; ++x) p[x] = o[x];
      }
      __syncthreads();
      for (int id = tid; id < NBLK * 8; id += 256) {   // forward along y, quantiser, inverse along v: a thread per block column
        const int blk = id >> 3, u = id & 7;
        int* p = s_d + blk * BLK + u;
        const int* Q = s_q + (blk >= 16 ? 64 : 0) + u;
        int a[8], F[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) a[y] = p[y * 9];
        dct8<false, 15>(a, F);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          const int Qv = Q[v * 8], m = abs(F[v]) + (Qv >> 1);
          // m < 2^15 and Qv <= 255: the fp32 estimate is within one of the quotient, and is then made exact
          int k = (int)((float)m * __builtin_amdgcn_rcpf((float)Qv));
          const int r = m - k * Qv;
          k += r >= Qv ? 1 : (r < 0 ? -1 : 0);
          F[v] = (F[v] < 0 ? -k : k) * Qv;
        }
        dct8<true, 9>(F, a);
#pragma unroll
        for (int y = 0; y < 8; ++y) p[y * 9] = a[y];
      }
      __syncthreads();
      for (int id = tid; id < NBLK * 8; id += 256) {   // inverse along u
        int* p = s_d + (id >> 3) * BLK + (id & 7) * 9;
        int a[8], o[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) a[x] = p[x];
        dct8<true, 15>(a, o);
#pragma unroll
        for (int x = 0; x < 8; ++x) p[x] = clampi(o[x] + 128, 0, 255);
      }
      __syncthreads();
      // triangle up-sampling of the chroma (edge replication at the padded plane's border), back to RGB
      const int Hc = ((H + 15) >> 4) << 3, Wc = ((W + 15) >> 4) << 3;   // the padded chroma plane
      const int cy0 = (ty0 - MARG) >> 1, cx0 = (tx0 - MARG) >> 1;        // plane coordinates of the region's chroma (0, 0)
      for (int idx = tid; idx < TILE * TILE; idx += 256) {
        const int y = idx >> 5, x = idx & 31, gy = ty0 + y, gx = tx0 + x;
        if (gy >= H || gx >= W) continue;
        const int i = gy >> 1, j = gx >> 1;
        const int i2 = clampi((gy & 1) ? i + 1 : i - 1, 0, Hc - 1), j2 = clampi((gx & 1) ? j + 1 : j - 1, 0, Wc - 1);
        const int li = clampi(i - cy0, 0, 31), li2 = clampi(i2 - cy0, 0, 31);
        const int lj = clampi(j - cx0, 0, 31), lj2 = clampi(j2 - cx0, 0, 31);
        const int o00 = ((li >> 3) * 4 + (lj >> 3)) * BLK + (li & 7) * 9 + (lj & 7);
        const int o10 = ((li2 >> 3) * 4 + (lj >> 3)) * BLK + (li2 & 7) * 9 + (lj & 7);
        const int o01 = ((li >> 3) * 4 + (lj2 >> 3)) * BLK + (li & 7) * 9 + (lj2 & 7);
        const int o11 = ((li2 >> 3) * 4 + (lj2 >> 3)) * BLK + (li2 & 7) * 9 + (lj2 & 7);
        const int bias = (gx & 1) ? 7 : 8;
        int cc[2];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
          const int* d = s_d + (16 + 16 * pl) * BLK;
          const int v0 = 3 * d[o00] + d[o10], v1 = 3 * d[o01] + d[o11];   // columns j and j2 after the vertical pass
          cc[pl] = ((3 * v0 + v1 + bias) >> 4) - 128;
        }
        const int Y = s_d[((y >> 3) * 4 + (x >> 3)) * BLK + (y & 7) * 9 + (x & 7)];
        unsigned char* o = s_px + idx * 3;
        o[0] = (unsigned char)clampi(Y + ((91881 * cc[1] + 32768) >> 16), 0, 255);
        o[1] = (unsigned char)clampi(Y + ((-22554 * cc[0] - 46802 * cc[1] + 32768) >> 16), 0, 255);
        o[2] = (unsigned char)clampi(Y + ((116130 * cc[0] + 32768) >> 16), 0, 255);
      }
    }
  }
  __syncthreads();
  // the tile's bytes [32][96] in s_px -> out: whole aligned dwords where a row has them, bytes at its ends
  const int rows = min(TILE, H - ty0), nb = 3 * min(TILE, W - tx0);
  for (int id = tid; id < rows * 25; id += 256) {
    const int y = id / 25, d = id - y * 25;
    const long g = fbase + ((long)(ty0 + y) * W + tx0) * 3;   // byte offset of the row's first byte
    const int mis = (int)((reinterpret_cast<uintptr_t>(out) + (unsigned long)g) & 3);
    const int j0 = 4 * d - mis;                                // the row byte at this aligned dword's byte 0
    const unsigned char* s = s_px + y * (TILE * 3);
    if (j0 >= 0 && j0 + 4 <= nb) {
      const unsigned v = (unsigned)s[j0] | ((unsigned)s[j0 + 1] << 8) | ((unsigned)s[j0 + 2] << 16) |
                         ((unsigned)s[j0 + 3] << 24);
      *reinterpret_cast<unsigned*>(out + g + j0) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j0 + e >= 0 && j0 + e < nb) out[g + j0 + e] = s[j0 + e];
    }
  }
}

}  // namespace

extern "C" {

// in, out [B][Tmax][H][W][3] uint8 (out must not alias in), len [B], tab [B][16] int32: include/xcp.h.
// Stream-ordered, no host read, no allocation.
int xcp_clip_degrade(const unsigned char* in, const int* len, const int* tab, unsigned char* out, int B, int Tmax, int H,
                     int W, hipStream_t st) {
  if (B <= 0 || Tmax <= 0) return XCP_OK;
  if (H <= 0 || W <= 0 || !in || !len || !tab || !out || in == out) return XCP_EINVAL;
  if ((long)H * W > 0x7fffffffL / 3) return XCP_EUNSUPPORTED;   // a frame's byte offsets and the noise counter fit int32
  const int tiles_y = (H + TILE - 1) / TILE, tiles_x = (W + TILE - 1) / TILE;
  const long blocks = (long)B * Tmax * tiles_y * tiles_x;
  if (blocks > 0x7fffffffL) return XCP_EUNSUPPORTED;
  hipLaunchKernelGGL(clip_degrade_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in, len, tab, out, Tmax, H, W,
                     tiles_y, tiles_x);
  return (int)hipGetLastError();
}

}  // extern "C"
