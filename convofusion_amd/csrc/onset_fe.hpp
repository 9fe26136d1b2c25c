// Audio onset detection (cfd_audio_onsets, cfd_audio.hip): Mel powers and frame energies -> onset frames -> the CSR pair cfd_motion_eval
// takes.  What the reference's Alignment.load_audio does with librosa 0.10 on the host (onset_strength, onset_detect(backtrack=False),
// feature.rms, onset_backtrack, frames_to_time), float32 for the spectra and the envelope, int32 frames, float64 times:
//   afe_frame_kernel    (audio_fe.hpp) per frame: ONE transform gives the 128 Mel powers and the frame's energy r[t]
//   ons_detect_kernel   per waveform, one workgroup: the clip's largest Mel power, dB, the envelope, its min / max, the normalisation, the two
//                       clipped windows per frame, the greedy `wait` pass, the energy minima, the backtrack, the compaction into the
//                       waveform's own slot
//   ons_csr_kernel      one workgroup: scans the counts over the waveforms, writes offsets, times and frames
// No atomics.  Every sum has one fixed order and max / min are exact in any order, so a call gives the same bits every time, and a waveform
// sees nothing of the others before the closing scan: its results do not depend on the batch.
//
// LDS of ons_detect_kernel, T <= ONS_MAX_T = 2048 frames (40 KB + the reduction scratch):
//   x     float [2048]   the envelope, then the normalised envelope
//   r     float [2048]   the frame energies
//   flag  int   [2048]   candidates, then the accepted (raw) onsets
//   pos   int   [2048]   inclusive sum scan of flag: an onset's place in the waveform's slot
//   pmin  int   [2048]   inclusive max scan of (i is an energy minimum ? i : -1): the largest minimum <= i
// Per-frame work is spread over the 1024 threads; the scans give each thread two consecutive entries.  Only the greedy pass is sequential:
// wave 0 takes 64 frames at a time, ballots their candidate bits and walks the set bits in order with `last` in a register, which is
// the reference's loop for any `wait`.
#pragma once
#include "audio_fe.hpp"

constexpr int ONS_THREADS = 1024;
constexpr int ONS_MAX_T = 2 * ONS_THREADS;
constexpr int ONS_WAVES = ONS_THREADS / 64;

struct OnsArgs {
  const float* melpow;        // [n_wave][T][n_mels]
  const float* rms;           // [n_wave][T]
  int T, n_mels;
  float amin, top_db;
  int lag, pad_frames;        // envelope[j] = mean_m max(0, D[m][j - pad + lag] - D[m][j - pad]) for j >= pad, else 0
  int pre_max, post_max, pre_avg, post_avg, wait;
  float delta;
  float* env_out;             // [n_wave][T] or null
  int32_t* slot_raw;          // [n_wave][T]: the waveform's raw onset frames, count[u] of them
  int32_t* slot_bt;           // [n_wave][T]: the same onsets moved back to the energy minimum
  int32_t* count;             // [n_wave]
};

template <bool MAX>
__device__ __forceinline__ int ons_op(int a, int b) { return MAX ? max(a, b) : a + b; }

// Inclusive scan of s[0 .. 2 ONS_THREADS) in place (sum, or max with identity -1); thread t owns s[2 t] and s[2 t + 1].  wsum: ONS_WAVES ints.
// The caller has synchronised behind its stores into s; the scan ends synchronised.
template <bool MAX>
__device__ inline void ons_scan(int* s, int* wsum, int tid) {
  const int ident = MAX ? -1 : 0;
  const int lane = tid & 63, wv = tid >> 6;
  const int a = s[2 * tid], b = ons_op<MAX>(a, s[2 * tid + 1]);
  int v = b;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v = ons_op<MAX>(o, v);
  }
  if (lane == 63) wsum[wv] = v;
  __syncthreads();
  int pre = ident;
  for (int i = 0; i < wv; ++i) pre = ons_op<MAX>(pre, wsum[i]);
  int excl = __shfl_up(v, 1);
  if (lane == 0) excl = ident;
  excl = ons_op<MAX>(pre, excl);
  s[2 * tid] = ons_op<MAX>(excl, a);
  s[2 * tid + 1] = ons_op<MAX>(excl, b);
  __syncthreads();
}

// power_to_db(S, ref=1.0, amin, top_db) as onset_strength calls it: 10 log10(max(amin, S)), clipped below at (the clip's largest) - top_db.
// The logarithm of the float32 power is evaluated in float64 and rounded once, so a dB value is the correctly rounded float32: the
// envelope is a mean of small differences of numbers near -50, and a 2-ulp log10f would be most of its error.
__device__ __forceinline__ float ons_db10(float S, float amin) { return (float)(10.0 * log10((double)fmaxf(amin, S))); }
__device__ __forceinline__ float ons_db(float S, float amin, float floor_db) { return fmaxf(ons_db10(S, amin), floor_db); }

__global__ void __launch_bounds__(ONS_THREADS) ons_detect_kernel(OnsArgs a) {
  __shared__ float x[ONS_MAX_T], r[ONS_MAX_T];
  __shared__ int flag[ONS_MAX_T], pos[ONS_MAX_T], pmin[ONS_MAX_T];
  __shared__ float redf[2][ONS_WAVES];
  __shared__ int redi[2][ONS_WAVES];
  __shared__ int wsum[ONS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = a.T;
  const long long u = blockIdx.x;
  const float* mp = a.melpow + u * T * a.n_mels;

  // the clip's largest Mel power (all >= 0), and the energies into LDS
  for (int t = tid; t < T; t += ONS_THREADS) r[t] = a.rms[u * T + t];
  float m = 0.f;
  for (long long i = tid; i < (long long)T * a.n_mels; i += ONS_THREADS) m = fmaxf(m, mp[i]);
  m = afe_wave_max(m);
  if (lane == 0) redf[0][wv] = m;
  __syncthreads();
  m = 0.f;
#pragma unroll
  for (int i = 0; i < ONS_WAVES; ++i) m = fmaxf(m, redf[0][i]);
  const float floor_db = ons_db10(m, a.amin) - a.top_db;

  // the envelope: one wave per frame in turn, lanes over the bands, a fixed xor tree
  for (int j = wv; j < T; j += ONS_WAVES) {
    const int i = j - a.pad_frames;
    float e = 0.f;
    if (i >= 0 && i + a.lag < T) {           // (wave-uniform)
      const float* row0 = mp + (long long)i * a.n_mels;
      const float* row1 = mp + (long long)(i + a.lag) * a.n_mels;
      float acc = 0.f;
      for (int k = lane; k < a.n_mels; k += 64)
        acc += fmaxf(0.f, ons_db(row1[k], a.amin, floor_db) - ons_db(row0[k], a.amin, floor_db));
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
      e = acc / (float)a.n_mels;
    }
    if (lane == 0) {
      x[j] = e;
      if (a.env_out) a.env_out[u * T + j] = e;
    }
  }
  __syncthreads();

  // min, max, any non-zero, any non-finite
  float mn = FLT_MAX, mx = -FLT_MAX;
  int any = 0, bad = 0;
  for (int t = tid; t < T; t += ONS_THREADS) {
    const float v = x[t];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    any |= v != 0.f;
    bad |= !isfinite(v);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, d));
    mx = fmaxf(mx, __shfl_xor(mx, d));
    any |= __shfl_xor(any, d);
    bad |= __shfl_xor(bad, d);
  }
  if (lane == 0) {
    redf[0][wv] = mn;
    redf[1][wv] = mx;
    redi[0][wv] = any;
    redi[1][wv] = bad;
  }
  __syncthreads();
  mn = FLT_MAX, mx = -FLT_MAX, any = 0, bad = 0;
#pragma unroll
  for (int i = 0; i < ONS_WAVES; ++i) {
    mn = fminf(mn, redf[0][i]);
    mx = fmaxf(mx, redf[1][i]);
    any |= redi[0][i];
    bad |= redi[1][i];
  }
  const bool dead = bad || !any;               // onset_detect: an all-zero or non-finite envelope has no onsets
  const float den = (mx - mn) + FLT_MIN;       // max(e - min e) + tiny: rounding is monotone, so the largest difference is max - min
  for (int t = tid; t < T; t += ONS_THREADS) x[t] = (x[t] - mn) / den;
  __syncthreads();

  // peak_pick's three conditions, both windows clipped to [0, T)
  for (int t = tid; t < ONS_MAX_T; t += ONS_THREADS) {
    int c = 0;
    if (t < T && !dead) {
      const float v = x[t];
      const int lo = max(t - a.pre_max, 0), hi = min(t + a.post_max, T);
      float wm = v;
      for (int i = lo; i < hi; ++i) wm = fmaxf(wm, x[i]);
      const int lo2 = max(t - a.pre_avg, 0), hi2 = min(t + a.post_avg, T);
      float s = 0.f;
      for (int i = lo2; i < hi2; ++i) s += x[i];
      const float mean = s / (float)(hi2 - lo2);
      c = v == wm && v >= mean + a.delta && v != 0.f;
    }
    flag[t] = c;
  }
  __syncthreads();

  // the greedy pass: a candidate is kept when it lies more than `wait` frames behind the last one kept
  if (wv == 0) {
    long long last = -(1LL << 40);
    for (int c0 = 0; c0 < T; c0 += 64) {
      const unsigned long long cand = __ballot(flag[c0 + lane] != 0);       // (c0 + lane < ONS_MAX_T; frames past T hold 0)
      unsigned long long rest = cand, keep = 0;
      while (rest) {                                                         // (wave-uniform)
        const int i = __ffsll((long long)rest) - 1;
        rest &= rest - 1;
        if ((long long)(c0 + i) > last + a.wait) {
          keep |= 1ULL << i;
          last = c0 + i;
        }
      }
      flag[c0 + lane] = (int)((keep >> lane) & 1ULL);
    }
  }
  __syncthreads();

  // places in the slot, and the largest energy minimum at or in front of every frame (frame 0 counts as one)
  for (int t = tid; t < ONS_MAX_T; t += ONS_THREADS) {
    pos[t] = flag[t];
    bool ismin = t == 0;
    if (t >= 1 && t <= T - 2) ismin = r[t] <= r[t - 1] && r[t] < r[t + 1];
    pmin[t] = ismin ? t : -1;
  }
  __syncthreads();
  ons_scan<false>(pos, wsum, tid);
  ons_scan<true>(pmin, wsum, tid);
  for (int t = tid; t < T; t += ONS_THREADS)
    if (flag[t]) {
      a.slot_raw[u * T + pos[t] - 1] = t;
      a.slot_bt[u * T + pos[t] - 1] = pmin[t];
    }
  if (tid == 0) a.count[u] = pos[ONS_MAX_T - 1];
}

struct OnsCsrArgs {
  const int32_t* count;       // [n_wave]
  const int32_t* slot_raw;    // [n_wave][T]
  const int32_t* slot_bt;
  int n_wave, T, capacity;
  int time_hop;
  double time_sr;             // time = (frame * time_hop) / time_sr, as frames_to_time computes it
  int32_t* onset_off;         // [n_wave + 1]
  double* onset_t;            // [capacity]
  int32_t* raw_out;           // [capacity] or null
  int32_t* bt_out;            // [capacity] or null
  int32_t* n_total;           // [1] or null
};

// The counts' scan over the waveforms, 2048 at a time with a running carry, and every waveform's slot copied to its segment: one wave
// per waveform in turn, lanes over its onsets.  (The host has refused a capacity below the largest possible total; the guard stays.)
__global__ void __launch_bounds__(ONS_THREADS) ons_csr_kernel(OnsCsrArgs a) {
  __shared__ int s[ONS_MAX_T];
  __shared__ int wsum[ONS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = 0;
  if (tid == 0) a.onset_off[0] = 0;
  for (int base = 0; base < a.n_wave; base += ONS_MAX_T) {
    for (int i = tid; i < ONS_MAX_T; i += ONS_THREADS) s[i] = base + i < a.n_wave ? a.count[base + i] : 0;
    __syncthreads();
    ons_scan<false>(s, wsum, tid);
    const int n_here = min(ONS_MAX_T, a.n_wave - base);
    for (int i = tid; i < n_here; i += ONS_THREADS) a.onset_off[base + i + 1] = min(carry + s[i], a.capacity);
    for (int i = wv; i < n_here; i += ONS_WAVES) {
      const int end = carry + s[i], begin = carry + (i ? s[i - 1] : 0);
      const long long src = (long long)(base + i) * a.T;
      for (int j = lane; j < end - begin; j += 64) {
        const int dst = begin + j;
        if (dst >= a.capacity) break;
        const int f = a.slot_bt[src + j];
        a.onset_t[dst] = (double)((long long)f * a.time_hop) / a.time_sr;
        if (a.bt_out) a.bt_out[dst] = f;
        if (a.raw_out) a.raw_out[dst] = a.slot_raw[src + j];
      }
    }
    const int total = s[ONS_MAX_T - 1];
    __syncthreads();                                                     // (s is refilled by the next round)
    carry += total;
  }
  if (tid == 0 && a.n_total) *a.n_total = carry;
}
