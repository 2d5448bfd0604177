// Train-time augmentation of the speech-commands classifiers on the device (train_speech_commands.py:60-68): the per-sample numpy /
// librosa pipeline  ChangeAmplitude -> ChangeSpeedAndPitchAudio -> FixAudioLength -> ToSTFT -> StretchAudioOnSTFT ->
// TimeshiftAudioOnSTFT -> FixSTFTDimension -> AddBackgroundNoiseOnSTFT -> ToMelSpectrogramFromSTFT  (transforms/transforms_wav.py:
// 34-78, transforms/transforms_stft.py:14-114) as four batched kernels.  A lane is one clip or one background clip; every random
// number is drawn on the host in the reference's order (audiopure_amd/transforms/augment.py) and arrives as a per-lane device array.
// Plain stores, no atomics, nothing allocated, no synchronise: two runs give equal bits.
#include <math.h>

#include "ap_common.h"
#include "ap_fft.h"
#include "ap_mel.h"

namespace ap {

// out[lane][j] = amp * interp(x, j * speed_fac) for j < n_interp, zero up to L_out (transforms_wav.py:60,77,44-47).  np.interp on
// xp = 0 .. len-1: slope (x[i+1] - x[i]) times the offset plus x[i]; a position past len-1 (the last ones of np.arange(0, len, fac)
// may lie in (len-1, len)) takes x[len-1].  The position j * speed_fac is np.arange's own float64 value.
__global__ __launch_bounds__(256) void aug_wave_kernel(const float *__restrict__ x, const int *__restrict__ len, const float *__restrict__ amp,
                                                       const double *__restrict__ speed_fac, const int *__restrict__ n_interp,
                                                       const int *__restrict__ speed_applied, float *__restrict__ out, int L_max, int L_out) {
  const int lane = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= L_out) return;
  const float *xl = x + (size_t)lane * L_max;
  const int n = min(max(len[lane], 0), L_max);
  const float a = amp[lane];
  float v = 0.f;
  if (!speed_applied[lane]) {
    if (j < n) v = a * xl[j];                           // a scaled copy: one rounding, numpy's
  } else if (n > 0 && j < n_interp[lane]) {
    const double pos = (double)j * speed_fac[lane];
    const int i = (int)floor(pos);
    if (!(pos >= 0.0)) v = a * xl[0];                   // (never with a positive factor; NaN lands here too)
    else if (i >= n - 1) v = a * xl[n - 1];
    else {
      const float x0 = xl[i], x1 = xl[i + 1];
      v = a * ((x1 - x0) * (float)(pos - (double)i) + x0);
    }
  }
  out[(size_t)lane * L_out + j] = v;
}

// librosa.stft(n_fft=2048, hop_length=512): centred frames, periodic Hann, bins 0..1024 of the 2048-point FFT, stored [lane][frame][bin]
// (the vocoder's per-bin walk over frames then reads neighbouring bins from neighbouring threads).  pad_mode 0: zeros; 1: reflect
// (t -> -t, t -> 2 (L-1) - t; L > 1024 keeps one reflection enough).
__global__ __launch_bounds__(256) void stft_kernel(const float *__restrict__ x, float2 *__restrict__ out, int reflect, int n_frames, int L) {
  __shared__ float2 bufA[NFFT];
  __shared__ float2 bufB[NFFT];
  __shared__ float2 tw[NFFT / 2];
  const int tid = threadIdx.x;
  const int frame = blockIdx.x, lane = blockIdx.y;
  const float *xb = x + (size_t)lane * L;
  for (int m = tid; m < NFFT / 2; m += 256) {
    float s, c;
    sincospif((float)m * (1.0f / 1024.0f), &s, &c);   // exp(-2 pi i m / 2048)
    tw[m] = make_float2(c, -s);
  }
  for (int n = tid; n < NFFT; n += 256) {
    int t = frame * HOP - NFFT / 2 + n;
    if (reflect) t = t < 0 ? -t : t >= L ? 2 * (L - 1) - t : t;
    const float v = (t >= 0 && t < L) ? xb[t] : 0.f;
    const float w = 0.5f - 0.5f * cospif((float)n * (1.0f / 1024.0f));   // periodic hann
    bufA[n] = make_float2(v * w, 0.f);
  }
  __syncthreads();
  const float2 *src = fft2048(bufA, bufB, tw, tid);
  float2 *o = out + ((size_t)lane * n_frames + frame) * NBIN;
  for (int k = tid; k < NBIN; k += 256) o[k] = src[k];
}

__device__ __forceinline__ float wrap_pi(float a) { return a - 6.2831853071795865f * rintf(a * 0.15915494309189534f); }

// librosa.core.phase_vocoder(D, rate, hop_length=512) + TimeshiftAudioOnSTFT + FixSTFTDimension (transforms_stft.py:44,59-67,89-98),
// one thread per (lane, bin).  The stretched STFT S has T = n_out columns (T = F where the stretch is not applied, S = D); the
// shift and the fix keep  out[:, c] = S[:, c + shift]  for c < min(T, F) with 0 <= c + shift < T  and zeros elsewhere.
// Vocoder step t reads columns i = floor(t rate), i + 1 of D padded with zeros:  mag = (1 - a) |D_i| + a |D_i+1|,
// S_t = mag e^{i acc}, acc += phi + wrap(arg D_i+1 - arg D_i - phi), acc_0 = arg D_0, phi = pi k / 2 for hop 512 of n_fft 2048 --
// a quarter turn times k, so modulo 2 pi it is (k mod 4) pi / 2 and acc stays wrapped to [-pi, pi]: float32 keeps its 1e-7 rad
// where librosa's unwrapped float32 sum (up to 6e4 rad) loses 1e-2.
__global__ __launch_bounds__(256) void phase_vocoder_shift_kernel(const float2 *__restrict__ D, float2 *__restrict__ out,
                                                                  const double *__restrict__ rate, const int *__restrict__ n_out,
                                                                  const int *__restrict__ stretch_applied, const int *__restrict__ shift,
                                                                  int F) {
  const int lane = blockIdx.y;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= NBIN) return;
  const float2 *Dl = D + (size_t)lane * F * NBIN + k;
  float2 *ol = out + (size_t)lane * F * NBIN + k;
  const bool applied = stretch_applied[lane] != 0;
  const int T = applied ? min(max(n_out[lane], 0), 4 * F) : F;
  const int sh = min(max(shift[lane], -F), F);
  const int keep = min(T, F);
  const float2 zero = make_float2(0.f, 0.f);
  if (!applied) {
    for (int c = 0; c < F; c++) {
      const int t = c + sh;
      ol[(size_t)c * NBIN] = (t >= 0 && t < T) ? Dl[(size_t)t * NBIN] : zero;     // a shifted copy
    }
    return;
  }
  for (int c = 0; c < F; c++) {
    const int t = c + sh;
    if (!(c < keep && t >= 0 && t < T)) ol[(size_t)c * NBIN] = zero;
  }
  const double r = rate[lane];
  const float phi = (float)(k & 3) * 1.5707963267948966f;
  const int t_end = min(T, keep + sh);                   // steps past the last surviving column are not walked
  const float2 d0 = Dl[0];
  float acc = atan2f(d0.y, d0.x);
  for (int t = 0; t < t_end; t++) {
    const double s = (double)t * r;
    const int i = (int)floor(s);
    const float alpha = (float)(s - (double)i);
    const float2 c0 = (i >= 0 && i < F) ? Dl[(size_t)i * NBIN] : zero;
    const float2 c1 = (i + 1 >= 0 && i + 1 < F) ? Dl[(size_t)(i + 1) * NBIN] : zero;
    const int c = t - sh;
    if (c >= 0 && c < keep) {
      const float mag = (1.0f - alpha) * sqrtf(c0.x * c0.x + c0.y * c0.y) + alpha * sqrtf(c1.x * c1.x + c1.y * c1.y);
      float sn, cs;
      sincosf(acc, &sn, &cs);
      ol[(size_t)c * NBIN] = make_float2(mag * cs, mag * sn);
    }
    const float dphase = wrap_pi(atan2f(c1.y, c1.x) - atan2f(c0.y, c0.x) - phi);
    acc = wrap_pi(acc + (phi + dphase));
  }
}

// AddBackgroundNoiseOnSTFT + ToMelSpectrogramFromSTFT before the per-clip maximum (transforms_stft.py:81-83,111-113): per (clip,
// frame)  D (1 - p) + D_noise p  (noise lane < 0: D as it is), |.|^2, the Slaney bank, 10 log10(max(., 1e-10)).
__global__ __launch_bounds__(256) void mel_from_stft_kernel(const float2 *__restrict__ D, const int *__restrict__ noise_lane,
                                                            const float *__restrict__ p, float *__restrict__ out, MelPts pts, int n_mels,
                                                            int n_lanes, int F) {
  __shared__ float pw[NBIN];
  const int tid = threadIdx.x;
  const int frame = blockIdx.x, b = blockIdx.y;
  const int nl = noise_lane[b];
  const float2 *d = D + ((size_t)b * F + frame) * NBIN;
  if (nl >= 0 && nl < n_lanes) {
    const float2 *dn = D + ((size_t)nl * F + frame) * NBIN;
    const float pn = p[b], pc = 1.0f - pn;
    for (int k = tid; k < NBIN; k += 256) {
      const float2 v = d[k], w = dn[k];
      const float re = v.x * pc + w.x * pn, im = v.y * pc + w.y * pn;
      pw[k] = re * re + im * im;
    }
  } else {
    for (int k = tid; k < NBIN; k += 256) {
      const float2 v = d[k];
      pw[k] = v.x * v.x + v.y * v.y;
    }
  }
  __syncthreads();
  if (tid < n_mels) {
    const float s = mel_filter_power(pts, pw, tid);
    out[((size_t)b * n_mels + tid) * F + frame] = 10.0f * log10f(fmaxf(s, 1e-10f));
  }
}

}  // namespace ap

extern "C" int ap_aug_wave(const float *x, const int32_t *len, const float *amp, const double *speed_fac, const int32_t *n_interp,
                           const int32_t *speed_applied, float *out, int N, int L_max, int L_out, void *stream) {
  using namespace ap;
  if (!x || !len || !amp || !speed_fac || !n_interp || !speed_applied || !out) { set_error("ap_aug_wave: null argument"); return -22; }
  if (N < 1 || N > 65535 || L_max < 1 || L_out < 1) { set_error("ap_aug_wave: N=%d L_max=%d L_out=%d", N, L_max, L_out); return -22; }
  if (x == out) { set_error("ap_aug_wave: out must not alias x"); return -22; }
  aug_wave_kernel<<<dim3((L_out + 255) / 256, N), 256, 0, (hipStream_t)stream>>>(x, len, amp, speed_fac, n_interp, speed_applied, out, L_max, L_out);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_stft(const float *x, float *out, int pad_mode, int N, int L, void *stream) {
  using namespace ap;
  if (!x || !out) { set_error("ap_stft: null argument"); return -22; }
  if (N < 1 || N > 65535 || L < 1) { set_error("ap_stft: N=%d L=%d", N, L); return -22; }
  if (pad_mode != AP_PAD_CONSTANT && pad_mode != AP_PAD_REFLECT) { set_error("ap_stft: pad_mode %d", pad_mode); return -22; }
  if (pad_mode == AP_PAD_REFLECT && L <= NFFT / 2) { set_error("ap_stft: reflect padding needs L > %d, got %d", NFFT / 2, L); return -22; }
  const int F = 1 + L / HOP;
  stft_kernel<<<dim3(F, N), 256, 0, (hipStream_t)stream>>>(x, (float2 *)out, pad_mode == AP_PAD_REFLECT, F, L);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_phase_vocoder_shift(const float *D, float *out, const double *rate, const int32_t *n_out, const int32_t *stretch_applied,
                                      const int32_t *shift, int N, int F, void *stream) {
  using namespace ap;
  if (!D || !out || !rate || !n_out || !stretch_applied || !shift) { set_error("ap_phase_vocoder_shift: null argument"); return -22; }
  if (N < 1 || N > 65535 || F < 1 || F > 4096) { set_error("ap_phase_vocoder_shift: N=%d F=%d", N, F); return -22; }
  if (D == out) { set_error("ap_phase_vocoder_shift: out must not alias D"); return -22; }
  phase_vocoder_shift_kernel<<<dim3((NBIN + 255) / 256, N), 256, 0, (hipStream_t)stream>>>((const float2 *)D, (float2 *)out, rate, n_out,
                                                                                           stretch_applied, shift, F);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_mel_from_stft(const float *D, const int32_t *noise_lane, const float *p, float *out, int n_mels, int B, int N, int F,
                                void *stream) {
  using namespace ap;
  if (!D || !noise_lane || !p || !out) { set_error("ap_mel_from_stft: null argument"); return -22; }
  if (B < 1 || N < B || N > 65535 || F < 1 || F > 65535) { set_error("ap_mel_from_stft: B=%d N=%d F=%d", B, N, F); return -22; }
  if (n_mels < 1 || n_mels > MAX_MELS) { set_error("ap_mel_from_stft: n_mels %d outside [1, %d]", n_mels, MAX_MELS); return -22; }
  MelPts pts;
  slaney_mel_points(&pts, n_mels);
  hipStream_t st = (hipStream_t)stream;
  mel_from_stft_kernel<<<dim3(F, B), 256, 0, st>>>((const float2 *)D, noise_lane, p, out, pts, n_mels, N, F);
  launch_mel_refmax(out, B, n_mels * F, st);
  AP_HIP(hipGetLastError());
  return 0;
}
