// The host side of stft / istft (afx_stft.h): the shapes taken, librosa's frame count and the statuses of a clip, istft's
// length rule, and the cost records afx_stft_batch / afx_istft_batch cut a batch with.  No device.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>

#include "afx.h"
#include "afx_internal.h"
#include "afx_stft.h"

namespace afx {

int stft_check_opts(const afx_stft_opts& o, const char** why) {
  auto fail = [&](int code, const char* w) { *why = w; return code; };
  if (o.n_fft != 1024 && o.n_fft != 2048) return fail(AFX_ERR_UNSUPPORTED, "n_fft must be 1024 or 2048");
  if (o.hop < 1 || o.hop > o.n_fft) return fail(AFX_ERR_UNSUPPORTED, "hop must be in [1, n_fft]");
  if (o.center != 0 && o.center != 1) return fail(AFX_ERR_INVALID, "center must be 0 or 1");
  if (o.pad_mode != AFX_PAD_CONSTANT && o.pad_mode != AFX_PAD_REFLECT) return fail(AFX_ERR_INVALID, "pad_mode must be AFX_PAD_CONSTANT or AFX_PAD_REFLECT");
  if (o.out_kind != AFX_STFT_COMPLEX && o.out_kind != AFX_STFT_MAG && o.out_kind != AFX_STFT_POWER) return fail(AFX_ERR_INVALID, "unknown out_kind");
  return AFX_OK;
}

void stft_frames(const afx_stft_opts& o, int64_t length, int64_t* T, int32_t* status) {
  const int64_t s = o.center ? o.n_fft / 2 : 0;
  const bool too_short = length == 0 || (!o.center && length < o.n_fft) ||
                         (o.center && o.pad_mode == AFX_PAD_REFLECT && length <= o.n_fft / 2);
  *status = too_short ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
  *T = too_short ? 0 : 1 + (length + 2 * s - o.n_fft) / o.hop;
}

void istft_samples(const afx_stft_opts& o, int64_t T, int64_t length, int64_t* n_frames, int64_t* n_out) {
  const int64_t s = o.center ? o.n_fft / 2 : 0;
  int64_t nf = T;
  if (length >= 0) nf = std::min<int64_t>(T, (length + 2 * s + o.hop - 1) / o.hop);
  *n_frames = nf;
  *n_out = length >= 0 ? length : nf > 0 ? o.n_fft + (int64_t)o.hop * (nf - 1) - 2 * s : 0;
}

void stft_cost(const afx_stft_opts& o, int sample_fmt, int mem_kind, int out_mem_kind, int inverse, StftCost& cost) {
  const int64_t bins = stft_bins(o.n_fft), hop = o.hop;
  cost = StftCost{};
  if (!inverse) {
    // a clip of L samples has at most 1 + L / hop frames: one row per clip and ceil(row / hop) bytes per sample hold them
    const int64_t row = out_mem_kind != AFX_MEM_HOST ? 0 : bins * (o.out_kind == AFX_STFT_COMPLEX ? 8 : 4);
    const int64_t up = mem_kind != AFX_MEM_HOST ? 0 : sample_fmt == AFX_FMT_S16 ? 2 : 4;
    cost.per_sample = 4 + up + (row + hop - 1) / hop;
    cost.per_clip = 256 + row + (int64_t)sizeof(StftClip) + (int64_t)sizeof(HpssClip);
  } else {
    // per frame used: its time row and (host) its spectrum row; per hop of output (host): the staged samples
    cost.per_sample = (int64_t)o.n_fft * 4 + (mem_kind == AFX_MEM_HOST ? bins * 8 : 0) + (out_mem_kind == AFX_MEM_HOST ? hop * 4 : 0);
    cost.per_clip = 256 + (int64_t)sizeof(IstftClip);
  }
  cost.tile = 16;
  cost.tile_cap = INT32_MAX / 2;
}

}  // namespace afx

using namespace afx;

static int stft_opts_arg(const char* who, const afx_stft_opts* opts) {
  if (!opts) { set_error(std::string(who) + ": null argument"); return AFX_ERR_INVALID; }
  const char* why = "";
  const int rc = stft_check_opts(*opts, &why);
  if (rc != AFX_OK) set_error(std::string(who) + ": " + why);
  return rc;
}

extern "C" int afx_stft_frames(const afx_stft_opts* opts, int64_t length, int64_t* T, int32_t* clip_status) {
  if (!T || !clip_status) { set_error("afx_stft_frames: null argument"); return AFX_ERR_INVALID; }
  if (int rc = stft_opts_arg("afx_stft_frames", opts)) return rc;
  if (length < 0 || length > (int64_t)1 << 31) { set_error("afx_stft_frames: length must be in [0, 2^31]"); return AFX_ERR_INVALID; }
  stft_frames(*opts, length, T, clip_status);
  return AFX_OK;
}

extern "C" int afx_istft_samples(const afx_stft_opts* opts, int64_t T, int64_t length, int64_t* n_frames, int64_t* n_out) {
  if (!n_frames || !n_out) { set_error("afx_istft_samples: null argument"); return AFX_ERR_INVALID; }
  if (int rc = stft_opts_arg("afx_istft_samples", opts)) return rc;
  if (T < 0 || T > (int64_t)1 << 31 || length > (int64_t)1 << 31) { set_error("afx_istft_samples: T must be in [0, 2^31] and length at most 2^31"); return AFX_ERR_INVALID; }
  istft_samples(*opts, T, length < 0 ? -1 : length, n_frames, n_out);
  return AFX_OK;
}

extern "C" int afx_stft_cost(const afx_stft_opts* opts, int sample_fmt, int mem_kind, int out_mem_kind, int inverse, int64_t* cost) {
  if (!cost) { set_error("afx_stft_cost: null argument"); return AFX_ERR_INVALID; }
  if ((sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) || (mem_kind != AFX_MEM_HOST && mem_kind != AFX_MEM_DEVICE) ||
      (out_mem_kind != AFX_MEM_HOST && out_mem_kind != AFX_MEM_DEVICE)) {
    set_error("afx_stft_cost: unknown sample format or memory kind");
    return AFX_ERR_INVALID;
  }
  if (int rc = stft_opts_arg("afx_stft_cost", opts)) return rc;
  StftCost c;
  stft_cost(*opts, sample_fmt, mem_kind, out_mem_kind, inverse != 0, c);
  const int64_t v[6] = {c.per_frame, c.per_tile, c.per_sample, c.per_clip, c.tile, c.tile_cap};
  std::memcpy(cost, v, sizeof(v));
  return AFX_OK;
}
