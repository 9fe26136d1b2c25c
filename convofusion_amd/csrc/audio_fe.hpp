// The log-Mel front end (cfd_audio_encode, cfd_audio.hip): waveform -> Mel power -> dB, float32 throughout.  What the reference's data
// loader does with librosa (melspectrogram + power_to_db(ref=np.max), util.normalize, amplitude_to_db per 16-frame chunk) as four kernels:
//   afe_peak_kernel    per waveform: max|y| of every chunk, the waveform's peak, the activity bits            (one workgroup per waveform)
//   afe_frame_kernel   per frame: window -> FFT -> power -> Mel, all inside one workgroup                      (one workgroup per frame)
//                      (for cfd_audio_onsets, onset_fe.hpp, also the frame's energy from the same power spectrum)
//   afe_max_kernel     per waveform: the largest Mel power (power_to_db's ref=np.max)                         (one workgroup per waveform)
//   afe_db_kernel      per output element: dB against the waveform's max, the top_db clip, the window slice
// No atomics anywhere; max is exact in any order, and every sum has one fixed order, so a call gives the same bits every time and a
// waveform's bits do not depend on the batch.
//
// The FFT.  A real frame of n_fft samples is packed as NC = n_fft / 2 complex points z[n] = x[2n] + i x[2n + 1], transformed by a
// radix-4 Stockham autosort FFT (one radix-2 pass at the end when log2 NC is odd) that ping-pongs between two LDS buffers, and unpacked
// with the post-twiddle X[k] = E[k] + exp(-2 pi i k / n_fft) O[k].  All twiddles come from ONE host table tw[k] = exp(-2 pi i k / n_fft),
// k < n_fft, computed in float64 and rounded once: the pass of length n and stride s (n s = NC) reads w^p, w^2p, w^3p as tw[2ps],
// tw[4ps], tw[6ps] -- no product of twiddles, no device sine.
//
// LDS.  Two float2 buffers of NC points (16 KB at n_fft = 2048) and the power spectrum (NC + 1 floats).  A pass reads x[t + j NC / 4]
// -- consecutive points over consecutive lanes -- and writes y[q + s (4p + j)], t = p s + q: at s = 1 a stride of 4 points, at s = 4
// four points every 16.  A float2 store is served in groups of 16 lanes over 32 dword banks (16 points), so unswizzled those two passes
// are 4-way conflicts.  Point i is therefore kept at i ^ (5 * ((i >> 4) & 3)): bits 4-5 of the index are XORed into bits 0-1 and into
// bits 2-3.  At s = 1 the 16 lanes of a group differ in bits 2-5 of i, at s = 4 in bits 0-1 and 4-5; after the XOR their low four bits
// are all distinct in both cases; from s = 16 on the lanes are consecutive anyway.  The XOR permutes inside aligned blocks of 16
// points, so the consecutive reads (32 lanes over 64 banks = 32 points) stay conflict-free as well.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

constexpr int AFE_THREADS = 256;
constexpr int AFE_RED_THREADS = 1024;
constexpr int AFE_MAX_WIN = 64;          // window starts travel as a kernel argument

__device__ __forceinline__ int afe_swz(int i) { return i ^ (5 * ((i >> 4) & 3)); }
__device__ __forceinline__ float2 afe_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// In-LDS complex FFT of NC points (forward, exp(-i ...)); x holds the input (swizzled), y is scratch.  Returns the buffer that holds the
// result (swizzled, natural order).  Every thread of the workgroup calls it; the caller has synchronised behind its stores into x.
template <int NC>
__device__ inline float2* afe_fft(float2* x, float2* y, const float2* __restrict__ tw, int tid) {
  int s = 1;
#pragma unroll
  for (int n = NC; n >= 4; n >>= 2, s <<= 2) {
    for (int t = tid; t < NC / 4; t += AFE_THREADS) {
      const int q = t & (s - 1), p = t / s;
      const float2 a = x[afe_swz(t)], b = x[afe_swz(t + NC / 4)], c = x[afe_swz(t + NC / 2)], d = x[afe_swz(t + 3 * NC / 4)];
      const float2 apc = make_float2(a.x + c.x, a.y + c.y), amc = make_float2(a.x - c.x, a.y - c.y);
      const float2 bpd = make_float2(b.x + d.x, b.y + d.y), bmd = make_float2(b.x - d.x, b.y - d.y);
      const float2 jbmd = make_float2(-bmd.y, bmd.x);              // i (b - d)
      const int o = q + s * 4 * p;
      y[afe_swz(o)] = make_float2(apc.x + bpd.x, apc.y + bpd.y);
      const float2 r1 = make_float2(amc.x - jbmd.x, amc.y - jbmd.y), r2 = make_float2(apc.x - bpd.x, apc.y - bpd.y),
                   r3 = make_float2(amc.x + jbmd.x, amc.y + jbmd.y);
      if (p == 0) {                                                 // w = 1: no product, as an exact twiddle deserves
        y[afe_swz(o + s)] = r1;
        y[afe_swz(o + 2 * s)] = r2;
        y[afe_swz(o + 3 * s)] = r3;
      } else {
        const int k = 2 * p * s;
        y[afe_swz(o + s)] = afe_cmul(tw[k], r1);
        y[afe_swz(o + 2 * s)] = afe_cmul(tw[2 * k], r2);
        y[afe_swz(o + 3 * s)] = afe_cmul(tw[3 * k], r3);
      }
    }
    __syncthreads();
    float2* z = x; x = y; y = z;
  }
  if (s < NC) {                                                     // one radix-2 pass is left: n = 2, s = NC / 2
    for (int t = tid; t < NC / 2; t += AFE_THREADS) {
      const float2 a = x[afe_swz(t)], b = x[afe_swz(t + NC / 2)];
      y[afe_swz(t)] = make_float2(a.x + b.x, a.y + b.y);
      y[afe_swz(t + NC / 2)] = make_float2(a.x - b.x, a.y - b.y);
    }
    __syncthreads();
    float2* z = x; x = y; y = z;
  }
  return x;
}

struct AfeFrameArgs {
  const float* wave;          // [n_wave][n_samples]
  const float* peak;          // [n_wave], or null: no normalisation
  long long n_samples, T;     // frames per waveform: 1 + n_samples / hop
  int hop, n_mels;
  const float2* tw;           // [n_fft]
  const float* window;        // [n_fft]
  const float* melfb;         // [n_mels][n_fft / 2 + 1]
  const int* mel_range;       // [n_mels][2] or null
  float* out;                 // POWER: [n_wave][T][n_fft / 2 + 1] power; else [n_wave][T][n_mels] Mel power
  float* rms;                 // Mel instance only, or null: [n_wave][T] frame energy (librosa.feature.rms(S=|stft|)) of the same transform
};

// Frame f of waveform u: samples f hop - n_fft / 2 ... + n_fft of the waveform (zero outside it: center=True, pad_mode="constant"), each
// divided by the waveform's peak where asked, times the window; |rfft|^2; the Mel powers, one wave per band in turn, lanes over the
// band's bins and a fixed xor tree.
template <int NC, bool POWER>
__global__ void __launch_bounds__(AFE_THREADS) afe_frame_kernel(AfeFrameArgs a) {
  __shared__ float2 buf0[NC], buf1[NC];
  __shared__ float pw[NC + 1];
  const int tid = threadIdx.x;
  const long long f = blockIdx.x;
  const int u = blockIdx.y;
  const float* y = a.wave + (long long)u * a.n_samples;
  float pk = 0.f;
  bool norm = false;
  if (a.peak) {
    pk = a.peak[u];
    norm = pk >= FLT_MIN;
  }
  const long long g0 = f * a.hop - NC;
  for (int n = tid; n < NC; n += AFE_THREADS) {
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const long long g = g0 + 2 * n + e;
      float s = (g >= 0 && g < a.n_samples) ? y[g] : 0.f;
      if (norm) s = s / pk;
      v[e] = s * a.window[2 * n + e];
    }
    buf0[afe_swz(n)] = make_float2(v[0], v[1]);
  }
  __syncthreads();
  const float2* Z = afe_fft<NC>(buf0, buf1, a.tw, tid);
  for (int k = tid; k <= NC; k += AFE_THREADS) {
    const float2 zk = Z[afe_swz(k & (NC - 1))], zm = Z[afe_swz((NC - k) & (NC - 1))];
    const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
    const float2 o = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
    const float2 to = afe_cmul(a.tw[k], o);
    const float xr = e.x + to.x, xi = e.y + to.y;
    const float p = xr * xr + xi * xi;
    if (POWER) a.out[((long long)u * a.T + f) * (NC + 1) + k] = p;
    else pw[k] = p;
  }
  if (POWER) return;
  __syncthreads();
  const int lane = tid & 63;
  for (int m = tid >> 6; m < a.n_mels; m += AFE_THREADS / 64) {
    int lo = 0, hi = NC + 1;
    if (a.mel_range) {                                             // a stray range stays inside the spectrum
      lo = max(a.mel_range[2 * m], 0);
      hi = min(a.mel_range[2 * m + 1], NC + 1);
    }
    const float* w = a.melfb + (long long)m * (NC + 1);
    float acc = 0.f;
    for (int k = lo + lane; k < hi; k += 64) acc = fmaf(w[k], pw[k], acc);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) a.out[((long long)u * a.T + f) * a.n_mels + m] = acc;
  }
  if (a.rms) {      // sqrt(2 (sum_k P[k] - P[0] / 2 - P[n_fft / 2] / 2) / n_fft^2): thread-strided partial sums, the xor tree, the waves in order
    __shared__ float red[AFE_THREADS / 64];
    float acc = 0.f;
    for (int k = tid; k <= NC; k += AFE_THREADS) acc += (k == 0 || k == NC) ? 0.5f * pw[k] : pw[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      float s = red[0];
#pragma unroll
      for (int i = 1; i < AFE_THREADS / 64; ++i) s += red[i];
      a.rms[(long long)u * a.T + f] = sqrtf(2.0f * s / ((float)(2 * NC) * (float)(2 * NC)));
    }
  }
}

__device__ __forceinline__ float afe_wave_max(float m) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  return m;
}

// max|y| per chunk of `chunk` samples (the last one may be partial) -> chunkmax [n_wave][n_chunks]; the waveform's peak -> peak_ws and,
// where given, peak_out; the activity bit of whole chunk j < n_bits: max(amin_p, (max|y| / peak)^2) > thresh -- division is monotone,
// so the largest sample of the normalised chunk is the chunk's largest sample normalised.
__global__ void __launch_bounds__(AFE_RED_THREADS) afe_peak_kernel(const float* __restrict__ wave, long long n_samples, int chunk, long long n_chunks,
                                                                   int normalize, float amin_p, float thresh, float* __restrict__ chunkmax,
                                                                   float* __restrict__ peak_ws, float* __restrict__ peak_out,
                                                                   int* __restrict__ activity, long long n_bits) {
  __shared__ float red[AFE_RED_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long u = blockIdx.x;
  const float* y = wave + u * n_samples;
  float* cm = chunkmax + u * n_chunks;
  float pk = 0.f;
  for (long long j = wv; j < n_chunks; j += AFE_RED_THREADS / 64) {
    const long long lo = j * chunk, hi = lo + chunk < n_samples ? lo + chunk : n_samples;
    float m = 0.f, mm[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    long long i = lo + lane;
    for (; i + 7 * 64 < hi; i += 8 * 64) {     // eight independent loads in flight per lane: one workgroup reads the whole waveform
#pragma unroll
      for (int e = 0; e < 8; ++e) mm[e] = fmaxf(mm[e], fabsf(y[i + e * 64]));
    }
    for (; i < hi; i += 64) m = fmaxf(m, fabsf(y[i]));
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, mm[e]);
    m = afe_wave_max(m);
    if (lane == 0) cm[j] = m;
    pk = fmaxf(pk, m);
  }
  if (lane == 0) red[wv] = pk;
  __syncthreads();
  pk = 0.f;
#pragma unroll
  for (int i = 0; i < AFE_RED_THREADS / 64; ++i) pk = fmaxf(pk, red[i]);
  if (tid == 0) {
    peak_ws[u] = pk;
    if (peak_out) peak_out[u] = pk;
  }
  if (!activity) return;
  const bool norm = normalize && pk >= FLT_MIN;
  for (long long j = tid; j < n_bits; j += AFE_RED_THREADS) {
    float m = cm[j];
    if (norm) m = m / pk;
    activity[u * n_bits + j] = fmaxf(amin_p, m * m) > thresh ? 1 : 0;
  }
}

// smax[u] = the largest of the waveform's T * n_mels Mel powers (all >= 0)
__global__ void __launch_bounds__(AFE_RED_THREADS) afe_max_kernel(const float* __restrict__ melpow, long long per_wave, float* __restrict__ smax) {
  __shared__ float red[AFE_RED_THREADS / 64];
  const int tid = threadIdx.x;
  const float* p = melpow + (long long)blockIdx.x * per_wave;
  float m = 0.f;
  for (long long i = tid; i < per_wave; i += AFE_RED_THREADS) m = fmaxf(m, p[i]);
  m = afe_wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    m = 0.f;
#pragma unroll
    for (int i = 0; i < AFE_RED_THREADS / 64; ++i) m = fmaxf(m, red[i]);
    smax[blockIdx.x] = m;
  }
}

struct AfeDbArgs {
  const float* melpow;        // [n_wave][T][n_mels]
  const float* smax;          // [n_wave]
  float* out;                 // [n_wave * n_rows_per_wave][frames][n_mels]
  long long T, total;         // total: elements of out
  int n_mels, frames, n_win;  // n_win 0: the whole spectrogram (frames = T)
  float amin, top_db;
  int start[AFE_MAX_WIN];
};

// power_to_db(S, ref=np.max, amin, top_db): 10 log10(max(amin, S)) - 10 log10(max(amin, max S)), then max(., max - top_db) -- the largest
// entry is S = max S itself, whose two terms are the same float, so the max is exactly 0 and the clip is at -top_db.
__global__ void __launch_bounds__(256) afe_db_kernel(AfeDbArgs a) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.total) return;
  const int m = (int)(idx % a.n_mels);
  const long long rt = idx / a.n_mels;
  const int t = (int)(rt % a.frames);
  const long long row = rt / a.frames;
  const int nw = a.n_win > 0 ? a.n_win : 1;
  const long long u = row / nw;
  const long long src = (a.n_win > 0 ? a.start[row % nw] : 0) + t;
  const float S = a.melpow[(u * a.T + src) * a.n_mels + m];
  const float v = 10.0f * log10f(fmaxf(a.amin, S)) - 10.0f * log10f(fmaxf(a.amin, a.smax[u]));
  a.out[idx] = fmaxf(v, 0.0f - a.top_db);
}
