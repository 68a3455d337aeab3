// predict_rule.h -- the write rule of the prediction output (include/mipgpu.h, mip_predict_device_ex)
// as one function, shared by the kernels that walk a device list (mip_predict.hip: MIP, Planar
// and DC items; mip_predict_angular.hip: angular items, three kernels of one body) and, with the argument rules of the flags
// word and of mip_predicted_frames_ex, by the host code.  No HIP dependency on the host side;
// unit-tested by tests/cpp/test_predict_rule.cpp.
#pragma once
#include "angular_plan.h"

namespace mipgpu {

// One list item, decoded and checked: on = it is written, reg = a regular (Planar / DC) item,
// only ever set with REGULAR.
struct Item {
  bool on, reg;
  int frame, x, y, w, h, sid, modes, mode, pitch;
  long long offset;
};

MIP_INTRA_HD bool pred_mode_is_angular(int mode) {
  return mode >= MIP_MODE_ANGULAR(MIP_ANGULAR_FIRST) && mode <= MIP_MODE_ANGULAR(MIP_ANGULAR_LAST);
}

// The write rule, item by item.  `a` gives the call (nframes, nctus, ctu_cols, out_samples,
// unavail [nctus * 5380], geo [5380] = shape | x << 8 | y << 16 inside the CTU: PredictArgs, or
// the host test's own), shape(s) the descriptor of shape s.  REGULAR / ANGULAR: the mode
// alternatives of MIP_PRED_REGULAR / MIP_PRED_ANGULAR.  Nothing but the item, a.unavail and a.geo
// is read, and those only at indexes the checks before them allow.
template <bool REGULAR, bool ANGULAR, class Args, class Shapes>
MIP_INTRA_HD Item pred_decode(const Args &a, const mip_pred_item &it, const Shapes &shape) {
  Item c{};
  c.on = c.reg = false;
  if (it.frame < 0 || it.frame >= a.nframes || it.cu < 0 || it.cu >= a.nctus * MIP_CUS_PER_CTU) return c;
  if (a.unavail[it.cu]) return c;
  const int ctu = it.cu / MIP_CUS_PER_CTU;
  const uint32_t g = a.geo[it.cu - ctu * MIP_CUS_PER_CTU];  // shape | x << 8 | y << 16 inside the CTU
  const mip_shape_desc sd = shape((int)(g & 0xffu));
  c.w = sd.w;
  c.h = sd.h;
  c.sid = sd.size_id;
  c.modes = sd.modes;
  const bool reg = REGULAR && (it.mode == MIP_MODE_PLANAR || it.mode == MIP_MODE_DC);  // every shape has both
  const bool ang = ANGULAR && pred_mode_is_angular(it.mode);                           // and all 65 of these
  if (!reg && !ang && (it.mode < 0 || it.mode >= 2 * c.modes)) return c;
  if (it.pitch < c.w || (it.pitch & 3) || (it.offset & 3) || it.offset < 0 || it.offset > a.out_samples) return c;
  if (a.out_samples - it.offset < (long long)(c.h - 1) * it.pitch + c.w) return c;
  c.frame = it.frame;
  c.x = 128 * (ctu % a.ctu_cols) + (int)((g >> 8) & 0xffu);
  c.y = 128 * (ctu / a.ctu_cols) + (int)((g >> 16) & 0xffu);
  c.mode = it.mode;
  c.pitch = it.pitch;
  c.offset = it.offset;
  c.reg = reg;
  c.on = true;
  return c;
}

// ---- host side: the flags word of mip_predict_device_ex / mip_predict_frames_ex
inline bool pred_flags_ok(unsigned flags) { return (flags & ~(MIP_PRED_REGULAR | MIP_PRED_ANGULAR)) == 0; }

// ---- host side: the argument rules mip_predicted_frames_ex adds to mip_predicted_frames'.  With
// the angular stage off the list and the bias are not looked at (the call is mip_predicted_frames);
// with it on they follow mip_angular_device's rules and *list receives the list.
enum PredictedExError { kPredictedExOk = 0, kPredictedExFlags, kPredictedExModes, kPredictedExBias };
inline PredictedExError predicted_ex_args(unsigned flags, const uint8_t *ang_modes, int ang_nmodes, int32_t ang_bias, AngList *list) {
  if (flags & ~MIP_CHAIN_ANGULAR) return kPredictedExFlags;
  if (!(flags & MIP_CHAIN_ANGULAR)) return kPredictedExOk;
  if (!ang_list(ang_modes, ang_nmodes, list)) return kPredictedExModes;
  if (!ang_bias_ok(ang_bias)) return kPredictedExBias;
  return kPredictedExOk;
}

}  // namespace mipgpu
