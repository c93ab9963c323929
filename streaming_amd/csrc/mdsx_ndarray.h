// Row header parse of dynamic ndarray columns ('ndarray', 'ndarray:<dtype>'), shared by the
// header kernels (mdsx_kernels.hip: mdsx_ndarray_meta / mdsx_ndarray_shapes) and the collate
// kernels (mdsx_collate.hip) -- NDArray.decode (encodings.py:270-305): [dtype id: u8 if dynamic]
// [ndim << 2 | shape dtype: u8][shape: ndim x u8/u16/u32/u64][values].
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mdsx_kernels {

__host__ __device__ __forceinline__ bool value_dtype_ok(uint32_t id) {
  return id == 8 || id == 9 || id == 16 || id == 17 || id == 18 || id == 32 || id == 33 ||
         id == 34 || id == 64 || id == 65 || id == 66;
}

__device__ __forceinline__ uint64_t read_uint(const uint8_t* p, int nbytes) {
  uint64_t v = 0;
  for (int b = 0; b < nbytes; ++b) v |= uint64_t(p[b]) << (8 * b);
  return v;
}

// What the header of one row says. bad: the reference's decode raises (then id, ndim and numel
// are as far as the parse got: callers report zeros for them).
struct NdRow {
  uint32_t id;    // value dtype id (encodings.py:131-143)
  uint32_t ndim;
  int64_t pos;    // byte offset of the values inside the row
  int64_t numel;  // element count (0 when bad)
  bool bad;
};

// Row p[0, len) of a column whose static value dtype id is dtype_id (0: the row carries it).
// kShapes: dims k < shape_cols are also written to shape_row[k] (before any of them is judged).
template <bool kShapes>
__device__ __forceinline__ NdRow ndarray_parse_row(const uint8_t* p, int64_t len, int dtype_id,
                                                   int32_t shape_cols, int64_t* shape_row) {
  int64_t pos = 0;
  bool bad = false;
  uint32_t id = uint32_t(dtype_id);
  if (id == 0) {
    if (len < 1) bad = true;
    else id = p[pos++];
    if (!bad && !value_dtype_ok(id)) bad = true;
  }
  uint32_t ndim = 0, code = 0;
  if (!bad) {
    if (pos + 1 > len) bad = true;
    else {
      const uint32_t byte = p[pos++];
      ndim = byte >> 2;
      code = byte & 3;
    }
  }
  // shape = frombuffer(data[index:index + ndim * sbytes], shape dtype): a truncated header
  // yields fewer dims (or raises when the tail is not whole dims); the values then start past
  // the end and are empty.
  const int sbytes = 1 << code;
  const int64_t want = int64_t(ndim) * sbytes;
  if (!bad && want > len - pos) {
    if ((len - pos) % sbytes) bad = true;
    else ndim = uint32_t((len - pos) / sbytes);
  }
  // numpy's size rule (PyArray_NewFromDescr): zero dims make the array empty, the product of
  // the non-zero dims times the item size must fit in intp; dims above intp max raise.
  const int64_t item = int64_t(id >> 3);
  int64_t prod = item;
  bool zero = false;
  if (!bad) {
    for (uint32_t k = 0; k < ndim; ++k) {
      const uint64_t dim = read_uint(p + pos + k * sbytes, sbytes);
      if (kShapes && int32_t(k) < shape_cols) shape_row[k] = int64_t(dim);
      if (dim > uint64_t(INT64_MAX)) { bad = true; break; }
      if (dim == 0) { zero = true; continue; }
      if (__builtin_mul_overflow(prod, int64_t(dim), &prod)) { bad = true; break; }
    }
    pos = pos + want < len ? pos + want : len;
  }
  const int64_t numel = (bad || zero) ? 0 : prod / item;
  // frombuffer(data[index:], dtype).reshape(shape): the value bytes must be exactly numel items
  if (!bad && (len - pos) != numel * item) bad = true;
  return NdRow{id, ndim, pos, bad ? 0 : numel, bad};
}

}  // namespace mdsx_kernels
