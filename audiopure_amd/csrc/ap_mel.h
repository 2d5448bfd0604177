// What the two Slaney mel-dB front-ends share: ap_mel.hip (waveform -> mel-dB) and ap_augment.hip (augmented STFT -> mel-dB).
#pragma once
#include <hip/hip_runtime.h>

namespace ap {

constexpr int NFFT = 2048, HOP = 512, NBIN = NFFT / 2 + 1, MAX_MELS = 128;

struct MelPts {
  float f[MAX_MELS + 2];   // filter corner frequencies in Hz (n_mels + 2 used)
};

// corners of librosa.filters.mel(sr=16000, n_fft=2048, n_mels) / torchaudio's mel_scale='slaney': n_mels + 2 points equally spaced
// on the Slaney mel scale from 0 to 8000 Hz (ap_mel.hip)
void slaney_mel_points(MelPts *pts, int n_mels);
// librosa.power_to_db(ref=np.max, top_db=80) on `rows` rows of n dB values, in place: mel_refmax_kernel (ap_mel.hip)
void launch_mel_refmax(float *out, int rows, int n, hipStream_t st);

#ifdef __HIPCC__
// filter m of the Slaney bank (triangle between corners m, m+1, m+2, area-normalised) on the power spectrum pw[NBIN]
__device__ __forceinline__ float mel_filter_power(const MelPts &pts, const float *pw, int m) {
  const float f0 = pts.f[m], f1 = pts.f[m + 1], f2 = pts.f[m + 2];
  const float binhz = 8000.0f / (float)(NBIN - 1);   // all_freqs = linspace(0, sr/2, n_freqs)
  int lo = (int)floorf(f0 / binhz), hi = (int)ceilf(f2 / binhz);
  lo = max(lo, 0);
  hi = min(hi, NBIN - 1);
  const float enorm = 2.0f / (f2 - f0);              // slaney area normalisation
  const float id = 1.0f / (f1 - f0), iu = 1.0f / (f2 - f1);
  float s = 0.f;
  for (int k = lo; k <= hi; k++) {
    const float fr = (float)k * binhz;
    const float w = fmaxf(0.f, fminf((fr - f0) * id, (f2 - fr) * iu));
    s = __builtin_fmaf(w * enorm, pw[k], s);
  }
  return s;
}
#endif

}  // namespace ap
