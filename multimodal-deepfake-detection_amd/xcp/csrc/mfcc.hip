// MFCC front end of the audio model (wavfake_audio_dataset.py:43: librosa.feature.mfcc(y, sr=16000,
// n_mfcc=13, n_fft=400, hop_length=160), then a slice of frames): padded PCM waveforms in, the
// [B, Tout, C, n_mfcc] input of XceptionLSTMA and the per-clip frame counts out.  Two launches on
// the caller's stream, nothing read back; the arithmetic contract (order of operations, what is
// rounded where) is the docstring of xcp/audio.py, whose mfcc_reference restates it in fp64.
//
// The window, the twiddles, the packed mel filterbank and the DCT rows are fp32 INPUTS (MfccPlan
// builds them in fp64 and rounds once): no kernel here evaluates a sine or a cosine.
//
// xcp_mfcc_logmel   one workgroup per run of RUN consecutive frames of one clip.  It stages the run's
//                   sample span (converted, times gain) in LDS once -- consecutive frames overlap by
//                   n_fft - hop samples --, the twiddles, and the windowed frames transposed to
//                   [n][RUN], so that the thread of bin k reads one twiddle pair per term (ds_read_b64)
//                   and applies it to all RUN frames (two broadcast ds_read_b128, 2 * RUN FMAs): the
//                   direct n_fft-term sum per (frame, bin), fp32, in index order.  Power, the sparse
//                   mel sums and 10 log10 follow in the workgroup; L goes to the workspace
//                   [B][Fmax][n_mels] and the run's maximum to wgmax[B][WGC].  No float atomics.
// xcp_mfcc_dct      one wave per output frame: the clip's maximum from wgmax, the top_db floor, the
//                   n_mfcc x n_mels product (each lane two bands, a butterfly sum: a fixed order),
//                   the C channel copies, zero rows past out_len, out_len itself.
#include "common.h"

#include <math.h>

namespace {

constexpr int MFCC_RUN = 8;          // frames a workgroup walks (fewer when hop is so large that the span would not fit)
constexpr int MFCC_THREADS = 256;
constexpr int MFCC_SPAN_MAX = 1792;  // floats of LDS for the sample span: (RUN - 1) hop + n_fft at the default config is 1520
constexpr int MFCC_NFFT_MAX = 1024, MFCC_NFFT_MIN = 16, MFCC_MELS_MAX = 128;
constexpr int MFCC_COLS = 4;         // XCP_MFCC_COLS: shift, f0, gain (fp32 bits), unused

struct MfccGeom {
  int Nmax, n_fft, hop, NB, Fmax, WGC, run;   // NB = n_fft / 2 + 1 bins, Fmax = 1 + Nmax / hop, WGC = ceil(Fmax / run)
};

__host__ __device__ inline int mfcc_run(int n_fft, int hop) {
  const long r = 1 + (long)(MFCC_SPAN_MAX - n_fft) / hop;
  return r < 1 ? 1 : (r > MFCC_RUN ? MFCC_RUN : (int)r);
}

// what the clip's table row and length say, clamped so that no load leaves wav[b, 0 .. Nmax)
struct ClipRow {
  int shift, f0, n, Fall;
  float gain;
};

XCP_DEV ClipRow clip_row(const int* len, const int* tab, int b, int Nmax, int hop) {
  ClipRow c;
  int L = len[b];
  L = L < 0 ? 0 : (L > Nmax ? Nmax : L);
  c.shift = 0; c.f0 = 0; c.gain = 1.f;
  if (tab) {
    const int s = tab[b * MFCC_COLS], f = tab[b * MFCC_COLS + 1];
    c.shift = s < 0 ? 0 : (s > Nmax ? Nmax : s);
    c.f0 = f < 0 ? 0 : f;
    c.gain = __int_as_float(tab[b * MFCC_COLS + 2]);
  }
  c.n = L - c.shift;
  c.Fall = c.n > 0 ? 1 + c.n / hop : 0;
  return c;
}

XCP_DEV float pcm(const float* w, long i) { return w[i]; }
XCP_DEV float pcm(const short* w, long i) { return (float)w[i] / 32768.f; }

XCP_DEV float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// LDS (dynamic): xwT [n_fft][RUN] | tw float2 [n_fft] | P [NB][RUN] | span [(run - 1) hop + n_fft] | red [4]
template <typename TW>
__global__ __launch_bounds__(MFCC_THREADS) void mfcc_logmel_kernel(
    const TW* __restrict__ wav, const int* __restrict__ len, const int* __restrict__ tab, const float* __restrict__ win,
    const float* __restrict__ tw_g, const int* __restrict__ mel_fc, const float* __restrict__ mel_w, int mel_pitch,
    float* __restrict__ Lws, float* __restrict__ wgmax, MfccGeom g, int n_mels, float amin) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xwT = smem;
  float2* tw = reinterpret_cast<float2*>(xwT + g.n_fft * MFCC_RUN);
  float* P = reinterpret_cast<float*>(tw + g.n_fft);
  float* span = P + g.NB * MFCC_RUN;
  float* red = span + ((g.run - 1) * g.hop + g.n_fft);

  const int tid = threadIdx.x;
  const int b = blockIdx.x / g.WGC, wg = blockIdx.x % g.WGC;
  const ClipRow c = clip_row(len, tab, b, g.Nmax, g.hop);
  const int f_lo = wg * g.run;
  int valid = c.Fall - f_lo;                      // frames of this run that exist
  valid = valid < 0 ? 0 : (valid > g.run ? g.run : valid);
  if (valid == 0) {                               // (uniform over the workgroup)
    if (tid == 0) wgmax[blockIdx.x] = -INFINITY;
    return;
  }

  // 1. the span y[f_lo hop - n_fft / 2 ...) of the valid frames, zero outside [0, n); twiddles
  const int span_len = (valid - 1) * g.hop + g.n_fft;
  const long base = (long)b * g.Nmax + c.shift;
  const int i0 = f_lo * g.hop - g.n_fft / 2;      // (f_lo <= Fmax, so f_lo hop <= Nmax + hop: no overflow for Nmax < 2^30)
  for (int s = tid; s < span_len; s += MFCC_THREADS) {
    const int i = i0 + s;
    span[s] = (i >= 0 && i < c.n) ? pcm(wav, base + i) * c.gain : 0.f;
  }
  for (int j = tid; j < g.n_fft; j += MFCC_THREADS) tw[j] = reinterpret_cast<const float2*>(tw_g)[j];
  __syncthreads();

  // 2. windowed frames, transposed: xwT[n][r] = y[(f_lo + r) hop - n_fft / 2 + n] w[n]
  for (int it = tid; it < g.n_fft * MFCC_RUN; it += MFCC_THREADS) {
    const int n = it / MFCC_RUN, r = it % MFCC_RUN;
    xwT[it] = r < valid ? span[r * g.hop + n] * win[n] : 0.f;
  }
  __syncthreads();

  // 3. X_k = sum_n xw[n] (cos - i sin)(2 pi k n / n_fft), entry (k n) mod n_fft of the table; P = re^2 + im^2
  const float4* xw4 = reinterpret_cast<const float4*>(xwT);
  for (int k = tid; k < g.NB; k += MFCC_THREADS) {
    float re[MFCC_RUN], im[MFCC_RUN];
#pragma unroll
    for (int r = 0; r < MFCC_RUN; ++r) re[r] = im[r] = 0.f;
    int idx = 0;
#pragma unroll 4
    for (int n = 0; n < g.n_fft; ++n) {
      const float2 t = tw[idx];
      const float4 a = xw4[2 * n], d = xw4[2 * n + 1];
      const float x[MFCC_RUN] = {a.x, a.y, a.z, a.w, d.x, d.y, d.z, d.w};
#pragma unroll
      for (int r = 0; r < MFCC_RUN; ++r) {
        re[r] = fmaf(x[r], t.x, re[r]);
        im[r] = fmaf(x[r], t.y, im[r]);
      }
      idx += k;
      if (idx >= g.n_fft) idx -= g.n_fft;
    }
#pragma unroll
    for (int r = 0; r < MFCC_RUN; ++r) P[k * MFCC_RUN + r] = re[r] * re[r] + im[r] * im[r];
  }
  __syncthreads();

  // 4. m_j = sum_k M[j][k] P_k over the filter's own bins, L_j = 10 log10(max(m_j, amin)); the run's maximum
  float mx = -INFINITY;
  for (int it = tid; it < valid * n_mels; it += MFCC_THREADS) {
    const int r = it / n_mels, j = it % n_mels;
    int first = mel_fc[2 * j], count = mel_fc[2 * j + 1];
    first = first < 0 ? 0 : (first > g.NB ? g.NB : first);
    const int room = g.NB - first < mel_pitch ? g.NB - first : mel_pitch;
    count = count < 0 ? 0 : (count > room ? room : count);
    const float* w = mel_w + (long)j * mel_pitch;
    float m = 0.f;
    for (int q = 0; q < count; ++q) m = fmaf(w[q], P[(first + q) * MFCC_RUN + r], m);
    const float L = 10.f * log10f(fmaxf(m, amin));
    Lws[((long)b * g.Fmax + f_lo + r) * n_mels + j] = L;
    mx = fmaxf(mx, L);
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) wgmax[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

constexpr int DCT_WAVES = 4;   // output frames per workgroup, one wave each

template <typename TO>
__global__ __launch_bounds__(DCT_WAVES * 64) void mfcc_dct_kernel(
    const float* __restrict__ Lws, const float* __restrict__ wgmax, const int* __restrict__ len, const int* __restrict__ tab,
    const float* __restrict__ dct, TO* __restrict__ out, int* __restrict__ out_len, MfccGeom g, int n_mels, int n_mfcc,
    int Tout, int C, int use_floor, float top_db, long rows) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * DCT_WAVES + (threadIdx.x >> 6);   // (b, t)
  if (row >= rows) return;                                              // (uniform over the wave)
  const int b = (int)(row / Tout), t = (int)(row % Tout);
  const ClipRow c = clip_row(len, tab, b, g.Nmax, g.hop);
  long avail = (long)c.Fall - c.f0;
  const int n_out = avail < 0 ? 0 : (avail > Tout ? Tout : (int)avail);
  if (t == 0 && lane == 0) out_len[b] = n_out;
  TO* o = out + row * C * n_mfcc;
  if (t >= n_out) {
    for (int i = lane; i < C * n_mfcc; i += 64) o[i] = from_f<TO>(0.f);
    return;
  }
  float lmax = -INFINITY;
  for (int w = lane; w < g.WGC; w += 64) lmax = fmaxf(lmax, wgmax[(long)b * g.WGC + w]);
  lmax = wave_max(lmax);
  const float floor_at = use_floor ? lmax - top_db : -INFINITY;
  const float* L = Lws + ((long)b * g.Fmax + c.f0 + t) * n_mels;
  const float l0 = lane < n_mels ? fmaxf(L[lane], floor_at) : 0.f;
  const float l1 = lane + 64 < n_mels ? fmaxf(L[lane + 64], floor_at) : 0.f;
  float c0 = 0.f, c1 = 0.f;   // lane i keeps coefficients i and i + 64
  for (int i = 0; i < n_mfcc; ++i) {
    const float* d = dct + (long)i * n_mels;
    float s = lane < n_mels ? d[lane] * l0 : 0.f;
    if (lane + 64 < n_mels) s = fmaf(d[lane + 64], l1, s);
    s = wave_sum(s);
    if ((i & 63) == lane) {
      if (i < 64) c0 = s; else c1 = s;
    }
  }
  for (int ch = 0; ch < C; ++ch) {
    if (lane < n_mfcc) o[ch * n_mfcc + lane] = from_f<TO>(c0);
    if (lane + 64 < n_mfcc) o[ch * n_mfcc + lane + 64] = from_f<TO>(c1);
  }
}

bool mfcc_geom(int B, int Nmax, int n_fft, int hop, int n_mels, MfccGeom* g) {
  if (B <= 0 || Nmax <= 0 || Nmax >= (1 << 30) || n_fft < MFCC_NFFT_MIN || n_fft > MFCC_NFFT_MAX || (n_fft & 1) || hop < 1 ||
      n_mels < 1 || n_mels > MFCC_MELS_MAX)
    return false;
  g->Nmax = Nmax; g->n_fft = n_fft; g->hop = hop; g->NB = n_fft / 2 + 1;
  g->Fmax = 1 + Nmax / hop;
  g->run = mfcc_run(n_fft, hop);
  g->WGC = (g->Fmax + g->run - 1) / g->run;
  return (long)B * g->WGC <= 0x7fffffffL;
}

size_t logmel_lds(const MfccGeom& g) {
  return sizeof(float) * ((size_t)g.n_fft * MFCC_RUN + 2 * (size_t)g.n_fft + (size_t)g.NB * MFCC_RUN +
                          (size_t)(g.run - 1) * g.hop + g.n_fft + 4);
}

}  // namespace

extern "C" {

// frames a workgroup of xcp_mfcc_logmel walks (8 unless hop is large); 0: unsupported n_fft / hop
int xcp_mfcc_run_frames(int n_fft, int hop) {
  MfccGeom g;
  return mfcc_geom(1, 1, n_fft, hop, 1, &g) ? g.run : 0;
}

// bytes of the workspace of the two kernels: L [B][Fmax][n_mels] fp32, then wgmax [B][WGC] fp32; -1: bad
// geometry or 2 GiB and more
int xcp_mfcc_ws_bytes(int B, int Nmax, int n_fft, int hop, int n_mels) {
  MfccGeom g;
  if (!mfcc_geom(B, Nmax, n_fft, hop, n_mels, &g)) return -1;
  const long bytes = 4 * ((long)B * g.Fmax * n_mels + (long)B * g.WGC);
  return bytes > 0x7fffffffL ? -1 : (int)bytes;
}

int xcp_mfcc_logmel(const void* wav, int wav_i16, const int* len, const int* tab, const float* win, const float* tw,
                    const int* mel_fc, const float* mel_w, int mel_pitch, float* ws, int B, int Nmax, int n_fft, int hop,
                    int n_mels, float amin, hipStream_t st) {
  MfccGeom g;
  if (!mfcc_geom(B, Nmax, n_fft, hop, n_mels, &g) || mel_pitch < 1 || xcp_mfcc_ws_bytes(B, Nmax, n_fft, hop, n_mels) < 0 ||
      !(amin > 0.f))
    return XCP_EINVAL;
  const size_t lds = logmel_lds(g);
  if (lds > 64 * 1024) return XCP_EUNSUPPORTED;   // (cannot happen inside the supported range: at most 63.0 KiB, at n_fft 1024)
  float* wgmax = ws + (long)B * g.Fmax * n_mels;
  const dim3 grid((unsigned)((long)B * g.WGC)), block(MFCC_THREADS);
  if (wav_i16)
    hipLaunchKernelGGL(mfcc_logmel_kernel<short>, grid, block, lds, st, (const short*)wav, len, tab, win, tw, mel_fc, mel_w,
                       mel_pitch, ws, wgmax, g, n_mels, amin);
  else
    hipLaunchKernelGGL(mfcc_logmel_kernel<float>, grid, block, lds, st, (const float*)wav, len, tab, win, tw, mel_fc, mel_w,
                       mel_pitch, ws, wgmax, g, n_mels, amin);
  return (int)hipGetLastError();
}

int xcp_mfcc_dct(const float* ws, const int* len, const int* tab, const float* dct, void* out, int* out_len, int B, int Nmax,
                 int n_fft, int hop, int n_mels, int n_mfcc, int Tout, int channels, int use_floor, float top_db, int dtype,
                 hipStream_t st) {
  MfccGeom g;
  if (!mfcc_geom(B, Nmax, n_fft, hop, n_mels, &g) || n_mfcc < 1 || n_mfcc > n_mels || Tout < 1 || channels < 1 ||
      (dtype != XCP_F32 && dtype != XCP_BF16) || (use_floor && !(top_db >= 0.f)))
    return XCP_EINVAL;
  const long rows = (long)B * Tout;
  const long blocks = (rows + DCT_WAVES - 1) / DCT_WAVES;
  if (blocks > 0x7fffffffL) return XCP_EUNSUPPORTED;
  const float* wgmax = ws + (long)B * g.Fmax * n_mels;
  const dim3 grid((unsigned)blocks), block(DCT_WAVES * 64);
  if (dtype == XCP_F32)
    hipLaunchKernelGGL(mfcc_dct_kernel<float>, grid, block, 0, st, ws, wgmax, len, tab, dct, (float*)out, out_len, g, n_mels,
                       n_mfcc, Tout, channels, use_floor, top_db, rows);
  else
    hipLaunchKernelGGL(mfcc_dct_kernel<bf16>, grid, block, 0, st, ws, wgmax, len, tab, dct, (bf16*)out, out_len, g, n_mels,
                       n_mfcc, Tout, channels, use_floor, top_db, rows);
  return (int)hipGetLastError();
}

}  // extern "C"
