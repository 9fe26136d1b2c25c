// libcfdenoise: the log-Mel front end -- waveforms to Mel frames in dB, AudioConvEncoder's memories and the activity bits in one call
// (cfd_audio_encode; kernels, the FFT and its LDS layout: audio_fe.hpp), its FFT stage alone (cfd_audio_power), and the audio onsets of
// the beat alignment as the CSR pair cfd_motion_eval takes (cfd_audio_onsets; onset_fe.hpp), and AudioConvEncoder's backward pass --
// the gradients of its weights, biases and Mel frames from the gradient at its output (cfd_audio_encoder_vjp; audio_enc_bwd.hpp).
#include "cfd_internal.hpp"
#include "audio_fe.hpp"
#include "onset_fe.hpp"
#include "audio_enc_bwd.hpp"

constexpr long long AFE_MAX_SAMPLES = 1LL << 26;

// What both entry points refuse about the transform itself
static int check_transform(const char* who, int n_wave, long long n_samples, int n_fft, int hop) {
  if (n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048)
    return fail(CFD_E_ARG, "%s: n_fft must be 256, 512, 1024 or 2048 (got %d)", who, n_fft);
  if (hop < 1) return fail(CFD_E_ARG, "%s: hop must be at least 1 (got %d)", who, hop);
  if (n_wave < 1 || n_wave > 65535) return fail(CFD_E_SHAPE, "%s: 1 <= n_wave <= 65535 (got %d)", who, n_wave);
  if (n_samples < 1 || n_samples > AFE_MAX_SAMPLES)
    return fail(CFD_E_SHAPE, "%s: 1 <= n_samples <= %lld (got %lld)", who, AFE_MAX_SAMPLES, n_samples);
  return CFD_OK;
}

template <bool POWER>
static int enqueue_frames(const AfeFrameArgs& f, int n_fft, int n_wave, hipStream_t st, int& launches) {
  const dim3 grid((unsigned)f.T, (unsigned)n_wave), block(AFE_THREADS);
  switch (n_fft) {
    case 256: LAUNCH_COUNTED(launches, (afe_frame_kernel<128, POWER>), grid, block, 0, st, f); break;
    case 512: LAUNCH_COUNTED(launches, (afe_frame_kernel<256, POWER>), grid, block, 0, st, f); break;
    case 1024: LAUNCH_COUNTED(launches, (afe_frame_kernel<512, POWER>), grid, block, 0, st, f); break;
    default: LAUNCH_COUNTED(launches, (afe_frame_kernel<1024, POWER>), grid, block, 0, st, f); break;
  }
  return CFD_OK;
}

// The Mel front of cfd_audio_encode and cfd_audio_onsets: the fields their argument structs share, wave to top_db, as one view; what
// both refuse about them; and their first stage, the peak launch where the call asks for one and the frame launch.
struct MelFront {
  const float* wave;
  int n_wave;
  long long n_samples;
  int normalize, n_fft, hop, n_mels;
  const float *twiddle, *window, *melfb;
  const int32_t* mel_range;
  float amin, top_db;
};
template <class A>
static MelFront mel_front_of(const A* a) {   // (a null struct gives null pointers, which check_mel_front refuses)
  if (!a) return MelFront{};
  return MelFront{a->wave, a->n_wave, a->n_samples, a->normalize, a->n_fft, a->hop, a->n_mels, a->twiddle, a->window, a->melfb, a->mel_range, a->amin, a->top_db};
}

// other_null: a pointer of the entry point's own that is refused in the same words
static int check_mel_front(const char* who, const MelFront& m, bool other_null = false) {
  if (other_null || !m.wave || !m.twiddle || !m.window || !m.melfb) return fail(CFD_E_ARG, "%s: bad argument (NULL pointer)", who);
  CHK(check_transform(who, m.n_wave, m.n_samples, m.n_fft, m.hop));
  if (m.n_mels < 1 || m.n_mels > m.n_fft / 2 + 1) return fail(CFD_E_ARG, "%s: 1 <= n_mels <= n_fft / 2 + 1 = %d (got %d)", who, m.n_fft / 2 + 1, m.n_mels);
  if (!(m.amin > 0.f) || !(m.top_db >= 0.f)) return fail(CFD_E_ARG, "%s: amin > 0 and top_db >= 0 (got %g, %g)", who, (double)m.amin, (double)m.top_db);
  if (m.normalize != 0 && m.normalize != 1) return fail(CFD_E_ARG, "%s: normalize is 0 or 1 (got %d)", who, m.normalize);
  return CFD_OK;
}

struct PeakAsk {   // what the peak launch takes beyond the front: the chunking, the activity bits and the caller's outputs
  int chunk;
  long long n_chunks;
  float act_amin_power, act_thresh_power;
  float *chunkmax, *peak_out;
  int* activity;
  long long n_bits;
};

// pk null: no peak launch; melpow null: no frame launch.  The frames are normalised by peak_ws where the front says so.
static int enqueue_mel_front(const MelFront& m, long long T, const PeakAsk* pk, float* peak_ws, float* melpow, float* rms, hipStream_t st, int& launches) {
  if (pk)
    LAUNCH_COUNTED(launches, afe_peak_kernel, dim3((unsigned)m.n_wave), dim3(AFE_RED_THREADS), 0, st, m.wave, m.n_samples, pk->chunk, pk->n_chunks,
                   m.normalize, pk->act_amin_power, pk->act_thresh_power, pk->chunkmax, peak_ws, pk->peak_out, pk->activity, pk->n_bits);
  if (!melpow) return CFD_OK;
  AfeFrameArgs f{};
  f.wave = m.wave; f.peak = m.normalize ? peak_ws : nullptr; f.n_samples = m.n_samples; f.T = T; f.hop = m.hop; f.n_mels = m.n_mels;
  f.tw = (const float2*)m.twiddle; f.window = m.window; f.melfb = m.melfb; f.mel_range = m.mel_range; f.out = melpow; f.rms = rms;
  return enqueue_frames<false>(f, m.n_fft, m.n_wave, st, launches);
}

extern "C" int cfd_audio_encode(cfd_handle c, const cfd_audio_args* a, float* mel_db, float* memory, int32_t* activity, float* peak,
                                void* stream) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  c->audio.launches = 0;
  const MelFront m = mel_front_of(a);
  CHK(check_mel_front("cfd_audio_encode", m));
  const bool mlp = a->w0 || a->b0 || a->w1 || a->b1 || a->w2 || a->b2;
  if (mlp && (!a->w0 || !a->b0 || !a->w1 || !a->b1 || !a->w2 || !a->b2 || a->hidden < 1 || a->latent < 1))
    return fail(CFD_E_ARG, "cfd_audio_encode: the encoder needs all of w0 b0 w1 b1 w2 b2 and hidden, latent >= 1 (got %d, %d)", a->hidden, a->latent);
  if (memory && !mlp) return fail(CFD_E_ARG, "cfd_audio_encode: memory asked for without the encoder's weights");
  if (activity && a->act_chunk < 1) return fail(CFD_E_ARG, "cfd_audio_encode: activity bits need act_chunk >= 1 (got %d)", a->act_chunk);
  const long long T = 1 + a->n_samples / a->hop;
  if (a->n_win < 0 || a->n_win > AFE_MAX_WIN) return fail(CFD_E_SHAPE, "cfd_audio_encode: 0 <= n_win <= %d (got %d)", AFE_MAX_WIN, a->n_win);
  long long frames = T;
  if (a->n_win > 0) {
    if (!a->win_start) return fail(CFD_E_ARG, "cfd_audio_encode: n_win = %d without win_start", a->n_win);
    if (a->win_frames < 1) return fail(CFD_E_SHAPE, "cfd_audio_encode: win_frames must be at least 1 (got %d)", a->win_frames);
    for (int w = 0; w < a->n_win; ++w)
      if (a->win_start[w] < 0 || (long long)a->win_start[w] + a->win_frames > T)
        return fail(CFD_E_SHAPE, "cfd_audio_encode: window %d = frames [%d, %lld) lies outside the %lld frames of a waveform", w, a->win_start[w],
                    (long long)a->win_start[w] + a->win_frames, T);
    frames = a->win_frames;
  }
  const long long rows = (long long)a->n_wave * (a->n_win > 0 ? a->n_win : 1);
  const long long out_rows = rows * frames;                      // rows of the dB matrix = rows of the MLP
  if (out_rows * a->n_mels > (1LL << 40) || (long long)a->n_wave * T * a->n_mels > (1LL << 40) || (memory && out_rows > 65535LL * 32))
    return fail(CFD_E_SHAPE, "cfd_audio_encode: too many frames for one call (%lld rows x %lld frames)", rows, frames);
  HIPCHK(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;

  const bool want_db = mel_db || memory;
  const bool front = a->normalize || peak || activity;
  const int chunk = a->act_chunk >= 1 ? a->act_chunk : 4096;
  const long long n_chunks = (a->n_samples + chunk - 1) / chunk, n_bits = a->act_chunk >= 1 ? a->n_samples / a->act_chunk : 0;
  float *chunkmax, *peak_ws, *smax, *melpow, *db_ws, *h1, *h2;
  CHK(carve(c->audio.ws, 64, [&](ArenaLayout& lay) {
    lay.take(chunkmax, front ? (size_t)(a->n_wave * n_chunks) : 0);
    lay.take(peak_ws, (size_t)a->n_wave);
    lay.take(smax, (size_t)a->n_wave);
    lay.take(melpow, want_db ? (size_t)a->n_wave * T * a->n_mels : 0);
    lay.take(db_ws, memory && !mel_db ? (size_t)out_rows * a->n_mels : 0);
    lay.take(h1, memory ? (size_t)out_rows * a->hidden : 0);
    lay.take(h2, memory ? (size_t)out_rows * a->latent : 0);
  }));
  c->audio.frames = T;
  c->audio.rows = rows;

  int launches = 0;
  const PeakAsk pk{chunk, n_chunks, a->act_amin_power, a->act_thresh_power, chunkmax, peak, (int*)activity, n_bits};
  CHK(enqueue_mel_front(m, T, front ? &pk : nullptr, peak_ws, want_db ? melpow : nullptr, nullptr, st, launches));
  if (want_db) {
    LAUNCH_COUNTED(launches, afe_max_kernel, dim3((unsigned)a->n_wave), dim3(AFE_RED_THREADS), 0, st, melpow, T * a->n_mels, smax);
    AfeDbArgs d{};
    float* db = mel_db ? mel_db : db_ws;
    d.melpow = melpow; d.smax = smax; d.out = db; d.T = T; d.total = out_rows * a->n_mels; d.n_mels = a->n_mels; d.frames = (int)frames;
    d.n_win = a->n_win; d.amin = a->amin; d.top_db = a->top_db;
    for (int w = 0; w < a->n_win; ++w) d.start[w] = a->win_start[w];
    LAUNCH_COUNTED(launches, afe_db_kernel, dim3((unsigned)((d.total + 255) / 256)), dim3(256), 0, st, d);
    if (memory) {                              // the three Linear layers on the library's float32 row kernel: K <= 512, a few thousand rows
      CHK(enqueue_linear_act(db, out_rows, a->n_mels, a->w0, a->b0, a->hidden, 2, h1, st));
      CHK(enqueue_linear_act(h1, out_rows, a->hidden, a->w1, a->b1, a->latent, 2, h2, st));
      CHK(enqueue_linear_act(h2, out_rows, a->latent, a->w2, a->b2, a->latent, 0, memory, st));
      launches += 3;
    }
  }
  c->audio.launches = launches;
  return CFD_OK;
}

// AudioConvEncoder's backward pass (audio_enc_bwd.hpp).  Launches: 2 for h1 and h2 (+ 1 with `out`), 1 for dz2 and 1 for dz1 where
// something below them is wanted, 1 for d_x, 1 for all wanted parameter gradients and 1 closing pass where the rows are more than one
// segment: 8 with everything wanted beyond 512 rows, 7 up to 512.
extern "C" int cfd_audio_encoder_vjp(cfd_handle c, const cfd_audio_enc_args* a, const float* d_out, float* out, float* const d_param[6], float* d_x,
                                     void* stream) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  c->audio_enc.launches = 0;
  if (!a) return fail(CFD_E_ARG, "cfd_audio_encoder_vjp: bad argument (NULL pointer)");
  float* dp[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool any_param = false;
  for (int i = 0; i < 6; ++i) {
    dp[i] = d_param ? d_param[i] : nullptr;
    any_param = any_param || dp[i];
  }
  if (!out && !d_x && !any_param) return fail(CFD_E_ARG, "cfd_audio_encoder_vjp: nothing is wanted (out, d_x and all six of d_param are NULL)");
  if (a->n_rows < 1 || a->n_rows > 65535LL * 32)
    return fail(CFD_E_SHAPE, "cfd_audio_encoder_vjp: 1 <= n_rows <= %lld (got %lld)", 65535LL * 32, a->n_rows);
  if (a->in_dim < 1 || a->in_dim > AEB_MAX_WIDTH || a->hidden < 1 || a->hidden > AEB_MAX_WIDTH || a->latent < 1 || a->latent > AEB_MAX_WIDTH)
    return fail(CFD_E_SHAPE, "cfd_audio_encoder_vjp: 1 <= in_dim, hidden, latent <= %d (got %d, %d, %d)", AEB_MAX_WIDTH, a->in_dim, a->hidden, a->latent);
  if (!a->x || !a->w0 || !a->b0 || !a->w1 || !a->b1 || !a->w2 || !a->b2 || !d_out)
    return fail(CFD_E_ARG, "cfd_audio_encoder_vjp: bad argument (NULL pointer: x, all of w0 b0 w1 b1 w2 b2 and d_out are needed)");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;

  const long long rows = a->n_rows;
  const int I = a->in_dim, H = a->hidden, D = a->latent;
  const bool need_dz1 = dp[0] || dp[1] || d_x, need_dz2 = need_dz1 || dp[2] || dp[3];
  const long long seg_rows = aeb_seg_rows(rows);
  const int n_seg = (int)((rows + seg_rows - 1) / seg_rows);
  const long long block[6] = {(long long)H * I, H, (long long)D * H, D, (long long)D * D, D};
  long long end[6], plane = 0;
  for (int i = 0; i < 6; ++i) end[i] = (plane += block[i]);
  float *h1, *h2, *dz2, *dz1, *planes;
  CHK(carve(c->audio_enc.ws, 64, [&](ArenaLayout& lay) {
    lay.take(h1, (size_t)rows * H);
    lay.take(h2, (size_t)rows * D);
    lay.take(dz2, need_dz2 ? (size_t)rows * D : 0);
    lay.take(dz1, need_dz1 ? (size_t)rows * H : 0);
    lay.take(planes, any_param && n_seg > 1 ? (size_t)n_seg * plane : 0);
  }));
  c->audio_enc.rows = rows;
  c->audio_enc.segments = n_seg;

  int launches = 0;
  CHK(enqueue_linear_act(a->x, rows, I, a->w0, a->b0, H, 2, h1, st));
  CHK(enqueue_linear_act(h1, rows, H, a->w1, a->b1, D, 2, h2, st));
  launches += 2;
  if (out) {
    CHK(enqueue_linear_act(h2, rows, D, a->w2, a->b2, D, 0, out, st));
    launches += 1;
  }
  const dim3 block256(AEB_THREADS);
  const unsigned gy = (unsigned)((rows + 31) / 32);
  if (need_dz2)
    LAUNCH_COUNTED(launches, aeb_dgrad_kernel<>, dim3((unsigned)((D + 63) / 64), gy), block256, 0, st, d_out, rows, D, a->w2, D, (const float*)h2, dz2);
  if (need_dz1)
    LAUNCH_COUNTED(launches, aeb_dgrad_kernel<>, dim3((unsigned)((H + 63) / 64), gy), block256, 0, st, (const float*)dz2, rows, D, a->w1, H, (const float*)h1, dz1);
  if (d_x)
    LAUNCH_COUNTED(launches, aeb_dgrad_kernel<>, dim3((unsigned)((I + 63) / 64), gy), block256, 0, st, (const float*)dz1, rows, H, a->w0, I, (const float*)nullptr, d_x);
  if (any_param) {
    AebWgradArgs w{};
    const float* g[3] = {dz1, dz2, d_out};
    const float* in[3] = {a->x, h1, h2};
    const int N[3] = {H, D, D}, K[3] = {I, H, D};
    int tiles = 0;
    for (int m = 0; m < 3; ++m) {
      AebLayer& y = w.layer[m];
      float *wd = dp[2 * m], *bd = dp[2 * m + 1];
      y.g = g[m]; y.a = in[m]; y.N = N[m]; y.K = K[m];
      if (n_seg > 1) {                                 // into the planes: block 2 m and 2 m + 1 of segment 0's
        y.w_dst = wd ? planes + (end[2 * m] - block[2 * m]) : nullptr;
        y.b_dst = bd ? planes + (end[2 * m + 1] - block[2 * m + 1]) : nullptr;
      } else {
        y.w_dst = wd; y.b_dst = bd;
      }
      y.nkt = wd ? (K[m] + AEB_TILE - 1) / AEB_TILE : 1;
      y.ntiles = wd || bd ? (N[m] + AEB_TILE - 1) / AEB_TILE * y.nkt : 0;
      tiles += y.ntiles;
    }
    w.n_rows = rows; w.seg_rows = seg_rows; w.seg_stride = n_seg > 1 ? plane : 0;
    LAUNCH_COUNTED(launches, aeb_wgrad_kernel<>, dim3((unsigned)tiles, (unsigned)n_seg), block256, 0, st, w);
    if (n_seg > 1) {
      AebCloseArgs k{};
      k.planes = planes; k.stride = plane; k.n_seg = n_seg;
      for (int i = 0; i < 6; ++i) { k.end[i] = end[i]; k.dst[i] = dp[i]; }
      LAUNCH_COUNTED(launches, aeb_close_kernel<>, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st, k);
    }
  }
  c->audio_enc.launches = launches;
  return CFD_OK;
}

extern "C" int cfd_audio_power(cfd_handle c, const float* wave, int n_wave, long long n_samples, int n_fft, int hop, const float* twiddle,
                               const float* window, float* power, void* stream) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  c->audio.launches = 0;
  if (!wave || !twiddle || !window || !power) return fail(CFD_E_ARG, "cfd_audio_power: bad argument (NULL pointer)");
  CHK(check_transform("cfd_audio_power", n_wave, n_samples, n_fft, hop));
  HIPCHK(hipSetDevice(c->cfg.device));
  AfeFrameArgs f{};
  f.wave = wave; f.n_samples = n_samples; f.T = 1 + n_samples / hop; f.hop = hop; f.tw = (const float2*)twiddle; f.window = window; f.out = power;
  int launches = 0;
  CHK(enqueue_frames<true>(f, n_fft, n_wave, (hipStream_t)stream, launches));
  c->audio.frames = f.T;
  c->audio.rows = n_wave;
  c->audio.launches = launches;
  return CFD_OK;
}

extern "C" int cfd_audio_onsets(cfd_handle c, const cfd_onset_args* a, int32_t* onset_off, double* onset_t, int32_t* n_total, void* stream) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  c->audio.launches = 0;
  const MelFront m = mel_front_of(a);
  CHK(check_mel_front("cfd_audio_onsets", m, !onset_off));
  if (a->lag < 1 || a->pad_frames < a->lag) return fail(CFD_E_ARG, "cfd_audio_onsets: lag >= 1 and pad_frames >= lag (got %d, %d)", a->lag, a->pad_frames);
  if (a->pre_max < 0 || a->pre_avg < 0 || a->wait < 0)
    return fail(CFD_E_ARG, "cfd_audio_onsets: pre_max, pre_avg and wait must not be negative (got %d, %d, %d)", a->pre_max, a->pre_avg, a->wait);
  if (a->post_max < 1 || a->post_avg < 1)       // (a window [n - pre, n + post) without frame n itself; post = 0 with pre = 0 is an empty one)
    return fail(CFD_E_ARG, "cfd_audio_onsets: post_max and post_avg must be at least 1 (got %d, %d)", a->post_max, a->post_avg);
  if (!(a->delta >= 0.f)) return fail(CFD_E_ARG, "cfd_audio_onsets: delta must not be negative (got %g)", (double)a->delta);
  if (a->time_hop < 1 || !(a->time_sr > 0.0)) return fail(CFD_E_ARG, "cfd_audio_onsets: time_hop >= 1 and time_sr > 0 (got %d, %g)", a->time_hop, a->time_sr);
  const long long T = 1 + a->n_samples / a->hop;
  if (T > ONS_MAX_T)
    return fail(CFD_E_SHAPE, "cfd_audio_onsets: %lld frames per waveform, the detection workgroup holds %d (n_samples < %lld at this hop)", T, ONS_MAX_T,
                (long long)ONS_MAX_T * a->hop);
  // two accepted onsets lie more than `wait` frames apart, so a waveform has at most ceil(T / (wait + 1)): the capacity is judged by that
  // bound, in front of the first launch, not by what the data turn out to hold
  const long long per_wave = (T + a->wait) / ((long long)a->wait + 1), worst = per_wave * a->n_wave;
  if (a->capacity < 0 || a->capacity < worst)
    return fail(CFD_E_SHAPE, "cfd_audio_onsets: capacity %d is below the %lld onsets %d waveforms of %lld frames can have at wait = %d", a->capacity, worst,
                a->n_wave, T, a->wait);
  if (worst > 0 && !onset_t) return fail(CFD_E_ARG, "cfd_audio_onsets: bad argument (NULL onset_t)");
  if ((long long)a->n_wave * T * a->n_mels > (1LL << 36))
    return fail(CFD_E_SHAPE, "cfd_audio_onsets: too many frames for one call (%d waveforms x %lld frames x %d bands)", a->n_wave, T, a->n_mels);
  HIPCHK(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;

  const int chunk = 4096;
  const long long n_chunks = (a->n_samples + chunk - 1) / chunk;
  float *chunkmax, *peak_ws, *melpow, *rms;
  int32_t *slot_raw, *slot_bt, *count;
  CHK(carve(c->audio.ws, 64, [&](ArenaLayout& lay) {
    lay.take(chunkmax, a->normalize ? (size_t)(a->n_wave * n_chunks) : 0);
    lay.take(peak_ws, (size_t)a->n_wave);
    lay.take(melpow, (size_t)a->n_wave * T * a->n_mels);
    lay.take(rms, a->rms ? 0 : (size_t)a->n_wave * T);
    lay.take(slot_raw, (size_t)a->n_wave * T);
    lay.take(slot_bt, (size_t)a->n_wave * T);
    lay.take(count, (size_t)a->n_wave);
  }));
  if (a->rms) rms = a->rms;
  c->audio.frames = T;
  c->audio.rows = a->n_wave;

  int launches = 0;
  const PeakAsk pk{chunk, n_chunks, 0.f, 0.f, chunkmax, nullptr, nullptr, 0};
  CHK(enqueue_mel_front(m, T, a->normalize ? &pk : nullptr, peak_ws, melpow, rms, st, launches));
  OnsArgs d{};
  d.melpow = melpow; d.rms = rms; d.T = (int)T; d.n_mels = a->n_mels; d.amin = a->amin; d.top_db = a->top_db; d.lag = a->lag; d.pad_frames = a->pad_frames;
  d.pre_max = a->pre_max; d.post_max = a->post_max; d.pre_avg = a->pre_avg; d.post_avg = a->post_avg; d.wait = a->wait; d.delta = a->delta;
  d.env_out = a->envelope; d.slot_raw = slot_raw; d.slot_bt = slot_bt; d.count = count;
  LAUNCH_COUNTED(launches, ons_detect_kernel, dim3((unsigned)a->n_wave), dim3(ONS_THREADS), 0, st, d);
  OnsCsrArgs s{};
  s.count = count; s.slot_raw = slot_raw; s.slot_bt = slot_bt; s.n_wave = a->n_wave; s.T = (int)T; s.capacity = a->capacity; s.time_hop = a->time_hop;
  s.time_sr = a->time_sr; s.onset_off = onset_off; s.onset_t = onset_t; s.raw_out = a->frames_raw; s.bt_out = a->frames; s.n_total = n_total;
  LAUNCH_COUNTED(launches, ons_csr_kernel, dim3(1), dim3(ONS_THREADS), 0, st, s);
  c->audio.launches = launches;
  return CFD_OK;
}
