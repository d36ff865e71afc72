// Host-side argument rules of the C entry points (include/idn.h), each worded once: plain C++, no
// HIP.  An entry point runs the rules that apply to it in its own order, which decides the error a
// caller sees (tests/test_abi_args.py pins it); a check only one entry point words stays there.
// Every rule returns an idn_status and leaves the text for idn_last_error().
#pragma once

#include "../../include/idn.h"

namespace idn {

int set_error(int status, const char* fmt, ...);  // abi.hip

inline int check_shape(const char* name, int n, int h, int w) {
  if (n >= 0 && h >= 1 && w >= 1) return IDN_OK;
  return set_error(IDN_EINVAL, "%s: bad shape n=%d h=%d w=%d", name, n, h, w);
}
inline int check_channels_1_or_3(const char* name, int c) {
  if (c == 1 || c == 3) return IDN_OK;
  return set_error(IDN_EINVAL, "%s: channels must be 1 or 3 (got %d)", name, c);
}
// c_text: how the message spells the channel count ("c", or the op's fixed "3" / "1")
inline int check_row_stride(const char* name, int64_t row_stride, int w, int c,
                            const char* c_text = "c") {
  if (row_stride >= (int64_t)w * c) return IDN_OK;
  return set_error(IDN_EINVAL, "%s: row_stride %lld < w*%s", name, (long long)row_stride, c_text);
}
inline int check_not_in_place(const char* name, const void* src, const void* dst,
                              const char* how = "src == dst", const char* what = "filtering") {
  if (src != dst) return IDN_OK;
  return set_error(IDN_EINVAL, "%s: in-place %s is not supported (%s)", name, what, how);
}
// src -> dst images: both pointers, in place, shape
inline int check_src_dst(const char* name, const void* src, const void* dst, int n, int h, int w,
                         const char* what = "filtering") {
  if (!src || !dst) return set_error(IDN_EINVAL, "%s: null pointer", name);
  if (int e = check_not_in_place(name, src, dst, "src == dst", what)) return e;
  return check_shape(name, n, h, w);
}
// shape, channels 1 or 3, stride: the order of the restoration ops
inline int check_image_1_or_3(const char* name, int n, int h, int w, int c, int64_t row_stride) {
  if (int e = check_shape(name, n, h, w)) return e;
  if (int e = check_channels_1_or_3(name, c)) return e;
  return check_row_stride(name, row_stride, w, c);
}
// the u8 -> u8 filters: check_src_dst, channels 1..4, stride
inline int check_filter_args(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                             int64_t row_stride, const char* name) {
  if (int e = check_src_dst(name, src, dst, n, h, w)) return e;
  if (c < 1 || c > 4) return set_error(IDN_EINVAL, "%s: channels must be 1..4 (got %d)", name, c);
  return check_row_stride(name, row_stride, w, c);
}
// A workspace of `need` bytes (0 asks for none), in the two wordings in use.  This one reports 0
// bytes for NULL and goes on to the 8-byte alignment, the order of every op that words it so.
inline int check_workspace(const char* name, const void* ws, size_t ws_bytes, size_t need) {
  if (!need) return IDN_OK;
  if (!ws || ws_bytes < need)
    return set_error(IDN_EWORKSPACE, "%s: workspace of %zu bytes needed, %zu given", name, need,
                     ws ? ws_bytes : (size_t)0);
  if ((uintptr_t)ws & 7) return set_error(IDN_EINVAL, "%s: workspace must be 8-byte aligned", name);
  return IDN_OK;
}
// ws_bytes as given, and the caller's status: IDN_EWORKSPACE in the wavelets and JPEG, IDN_EINVAL
// in quant and the coloured NL-means
inline int check_workspace_got(const char* name, const void* ws, size_t ws_bytes, size_t need,
                               int status) {
  if (!need || (ws && ws_bytes >= need)) return IDN_OK;
  return set_error(status, "%s: needs %zu workspace bytes (got %zu)", name, need, ws_bytes);
}
inline int batch_too_large(const char* name) {  // the caller owns the condition
  return set_error(IDN_EUNSUPPORTED, "%s: batch too large for one launch", name);
}

constexpr size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Carves a workspace: take(bytes) is the offset of the next region; total moves past it to the
// next multiple of `align`.  An op's layout function is one sequence of take() calls, read by its
// *_workspace_size (total) and by its entry point (the offsets): the two cannot disagree.
struct Bump {
  size_t align = 1, total = 0;
  size_t take(size_t bytes) {
    const size_t off = total;
    total = align_up(total + bytes, align);
    return off;
  }
};

}  // namespace idn
