// Device entry points of the HOST-ONLY build (libafx_host_asan.so, `make asan`): every one fails loudly with
// AFX_ERR_NO_DEVICE.  The sanitizer build exists to run the host-side parsers and table builders (afx_wav.cpp,
// afx_tables.cpp, afx_f0_tables.cpp, afx_resample_tables.cpp, afx_filt_host.cpp, afx_beat_host.cpp, afx_assess_host.cpp, afx_cfft_host.cpp, afx_smooth_host.cpp, afx_loudness_host.cpp, afx_gate_host.cpp, afx_stft_host.cpp, afx_pvoc_host.cpp, afx_host.cpp) under AddressSanitizer + UBSan on the CPU; GPU sanitizers are not
// available on the target pool.  Never linked into libafx.so.
#include <cstddef>
#include <cstdint>

#include "afx.h"
#include "afx_internal.h"

static int no_device(const char* who) {
  afx::set_error(std::string(who) + ": host-only sanitizer build of libafx (no device code)");
  return AFX_ERR_NO_DEVICE;
}

extern "C" {
int afx_device_count(void) { return 0; }
int afx_init(int, afx_ctx** out) { if (out) *out = nullptr; return no_device("afx_init"); }
void afx_destroy(afx_ctx*) {}
int afx_malloc(afx_ctx*, size_t, void**) { return no_device("afx_malloc"); }
int afx_free(afx_ctx*, void*) { return no_device("afx_free"); }
int afx_host_alloc(afx_ctx*, size_t, void** out) { if (out) *out = nullptr; return no_device("afx_host_alloc"); }
int afx_host_free(afx_ctx*, void*) { return no_device("afx_host_free"); }
int afx_memcpy_h2d(afx_ctx*, void*, const void*, size_t) { return no_device("afx_memcpy_h2d"); }
int afx_memcpy_d2h(afx_ctx*, void*, const void*, size_t) { return no_device("afx_memcpy_d2h"); }
int afx_synchronize(afx_ctx*) { return no_device("afx_synchronize"); }
int afx_plan_create(afx_ctx*, const afx_params*, afx_plan** out) { if (out) *out = nullptr; return no_device("afx_plan_create"); }
void afx_plan_destroy(afx_plan*) {}
int afx_extract_batch(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, float*, int32_t*, int64_t*,
                      int32_t*, float*, const int64_t*) { return no_device("afx_extract_batch"); }
int afx_extract_submit(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, float*, int32_t*, int64_t*,
                       int32_t*, float*, const int64_t*) { return no_device("afx_extract_submit"); }
int afx_extract_collect(afx_plan*) { return no_device("afx_extract_collect"); }
int afx_f0_batch(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, double, double, double*, int32_t*,
                 double*, const int64_t*) { return no_device("afx_f0_batch"); }
int afx_zcr_batch(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, double*, const int64_t*,
                  int32_t*) { return no_device("afx_zcr_batch"); }
int afx_spectral_batch(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, float*, const int64_t*,
                       int32_t*) { return no_device("afx_spectral_batch"); }
int afx_preprocess(afx_plan*, const float*, int64_t, float*, int64_t*, int64_t*, int32_t*) { return no_device("afx_preprocess"); }
int afx_plan_set_timing(afx_plan*, int) { return no_device("afx_plan_set_timing"); }
int afx_plan_get_timings(afx_plan*, float*, int32_t*, int) { return no_device("afx_plan_get_timings"); }
int afx_plan_get_intervals(afx_plan*, int, double*, double*, int, int32_t*) { return no_device("afx_plan_get_intervals"); }
int afx_dtw_batch(afx_ctx*, const float*, int, const int64_t*, const int64_t*, const int64_t*, const int64_t*, const int32_t*,
                  int, int, int, double*, int32_t*, int32_t*, const int64_t*, int32_t*, double*, const int64_t*) {
  return no_device("afx_dtw_batch");
}
int afx_dtw_steps_batch(afx_ctx*, const float*, int, const int64_t*, const int64_t*, const int64_t*, const int64_t*,
                        const int32_t*, int, int, int, const int32_t*, int, const double*, const double*, double*, int32_t*,
                        int32_t*, const int64_t*, int32_t*, double*, const int64_t*, int32_t*) {
  return no_device("afx_dtw_steps_batch");
}
int afx_hpss_batch(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, float*, float*, double*, float*,
                   const int64_t*, int32_t*) {
  return no_device("afx_hpss_batch");
}
int afx_chroma_batch(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, const double*, float*,
                     const int64_t*, float*, const int64_t*, double*, double*, int32_t*, int32_t*) {
  return no_device("afx_chroma_batch");
}
int afx_rhythm_batch(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, float*, const int64_t*, float*,
                     const int64_t*, double*, double*, int32_t*, double*, int32_t*) {
  return no_device("afx_rhythm_batch");
}
int afx_groups_batch(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, int, double*, double*, int32_t*,
                     int32_t*) {
  return no_device("afx_groups_batch");
}
int afx_beat_batch(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, const double*, double, int, uint8_t*,
                   const int64_t*, int32_t*, double*, int32_t*, float*, double*, double*, int32_t*, int32_t*) {
  return no_device("afx_beat_batch");
}
int afx_denoise_batch(afx_plan*, const void*, int, int, const int64_t*, const int64_t*, int, int, int, double, int, float*,
                      double*, int32_t*) {
  return no_device("afx_denoise_batch");
}
int afx_groups_debug_rows(afx_plan*, float*, int64_t, int64_t*) { return no_device("afx_groups_debug_rows"); }
int afx_resample_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, int, int, int, const double*, int, float*,
                       int, const int64_t*, int64_t*) {
  return no_device("afx_resample_batch");
}
int afx_decode_batch(afx_ctx*, const void*, int, const int64_t*, const int64_t*, const int32_t*, const int32_t*, int, float*, int,
                     const int64_t*) {
  return no_device("afx_decode_batch");
}
int afx_sosfiltfilt_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, int, const double*, int, int, int, float,
                          float*, int, const int64_t*, double*, int32_t*) {
  return no_device("afx_sosfiltfilt_batch");
}
int afx_assess_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, const int32_t*, const int32_t*, int, double,
                     int64_t, double*, int32_t*) {
  return no_device("afx_assess_batch");
}
int afx_compare_batch(afx_ctx*, const void*, const void*, int, int, const int64_t*, const int64_t*, const int64_t*, const int64_t*,
                      int, double*, int32_t*) {
  return no_device("afx_compare_batch");
}
int afx_specdist_batch(afx_ctx*, const void*, const void*, int, int, const int64_t*, const int64_t*, const int64_t*, const int64_t*,
                       int, double*, int32_t*) {
  return no_device("afx_specdist_batch");
}
int afx_clip_fft_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, int, double*, const int64_t*, int32_t*) {
  return no_device("afx_clip_fft_batch");
}
int afx_medfilt_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, int, int, float*, int, const int64_t*,
                      int32_t*) {
  return no_device("afx_medfilt_batch");
}
int afx_savgol_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, int, int, int, int, double, float*, int,
                     const int64_t*, int32_t*) {
  return no_device("afx_savgol_batch");
}
int afx_energy_zcr_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, int, int, int, int, int, double*,
                         int32_t*) {
  return no_device("afx_energy_zcr_batch");
}
int afx_loudness_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, const int32_t*, int, double, int, double,
                       double*, double*, const int64_t*, float*, int, const int64_t*, int32_t*) {
  return no_device("afx_loudness_batch");
}
int afx_gate_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, int, const int64_t*, const int64_t*,
                   const afx_gate_opts*, float*, int, const int64_t*, double*, uint32_t*, int32_t*) {
  return no_device("afx_gate_batch");
}
int afx_stft_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, int, const afx_stft_opts*, const float*, void*,
                   int, const int64_t*, int32_t*) {
  return no_device("afx_stft_batch");
}
int afx_istft_batch(afx_ctx*, const void*, int, const int64_t*, const int64_t*, int, const afx_stft_opts*, const float*,
                    const int64_t*, float*, int, const int64_t*, int32_t*) {
  return no_device("afx_istft_batch");
}
int afx_pvoc_batch(afx_ctx*, const void*, int, const int64_t*, const int64_t*, const double*, int, int, int, void*, int,
                   const int64_t*, int32_t*) {
  return no_device("afx_pvoc_batch");
}
int afx_time_stretch_batch(afx_ctx*, const void*, int, int, const int64_t*, const int64_t*, const double*, int, const afx_stft_opts*,
                           const float*, float*, int, const int64_t*, int32_t*) {
  return no_device("afx_time_stretch_batch");
}
}
