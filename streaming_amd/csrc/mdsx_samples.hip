// Many samples' bytes decoded exactly as MDSReader.decode_sample slices them (gfx950), in two
// launches and straight into device batch columns: mdsx_decode_samples_sizes /
// mdsx_decode_samples_copy, the batched form of mdsx_decode_sample (mdsx_sample.hip).
//
// The device batch path of a shard that breaks the MDS layout serves the samples the whole-shard
// decode refuses from here (order.DeviceSampleGather, malformed='reference'): each is read as the
// reference reads it (get_sample_data, mds/reader.py:128-149), and every column gets the slice
// the reference hands it (mds/reader.py:103-126): data[idx:idx + size], clipped, never an error.
// What the column's decoder then does with a short slice (numpy raises for int, scalars and static
// ndarrays; bytes.decode raises on a cut sequence) is the status / flag the caller reads.
//
// One wave per sample, as in decode_sample_kernel: lane c parses column c's head and size, a wave
// prefix places the columns (starts summed in 64 bits, clipped to the sample). Pass 1 writes the
// clipped length of every ragged column and the sample's status; the caller turns the lengths
// into offsets (a prefix sum per column) and sizes the value buffers; pass 2 parses again and
// copies every slice (wave_copy; its kUtf8 form for str columns, whose flag it writes) to its
// place. Neighbouring samples' outputs are adjacent: wave_copy stores whole 16-byte chunks only
// inside [dst, dst + len) and the partial chunks at both ends one byte per lane.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mdsx_decode.h"
#include "mdsx_device.h"
#include "mdsx_internal.h"

namespace mdsx_kernels {
namespace {

constexpr int kSampleWaves = 4;  // samples (waves) per workgroup
constexpr uint64_t kSampleSlack = 64;

struct SamplesPlan {
  int32_t ncols;
  int32_t nvar;
  uint32_t row_bytes[MDSX_MAX_COLUMNS];
  int8_t var_index[MDSX_MAX_COLUMNS];
  int8_t kind[MDSX_MAX_COLUMNS];
};

struct SamplesIn {
  const uint8_t* data;       // the buffer holding every sample
  uint64_t data_bytes;
  const uint64_t* offsets;   // [m] byte offset of sample k in data
  const uint32_t* bytes;     // [m] its length
  uint64_t m;
};

struct SizesArgs {
  SamplesIn in;
  SamplesPlan plan;
  int64_t* lengths;  // [nvar][m + 1]: lengths[v][k + 1] = clipped length (lengths[v][0] untouched)
  int32_t* status;   // [m][2]: status, column
};

struct CopyArgs {
  SamplesIn in;
  SamplesPlan plan;
  uint8_t* out[MDSX_MAX_COLUMNS];            // fixed: [m][row_bytes]; ragged: values
  const int64_t* offsets[MDSX_MAX_COLUMNS];  // ragged: [m + 1]
  uint8_t* flags[MDSX_MAX_COLUMNS];          // str: [m] (may be null)
  uint64_t capacity[MDSX_MAX_COLUMNS];       // ragged: bytes of values
};

// A value every lane holds alike, as a scalar (the copies below branch and address on it).
__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(x));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(x >> 32));
  return (uint64_t(hi) << 32) | lo;
}

// This wave's place in its workgroup, as a scalar: what follows branches on the sample it picks.
__device__ __forceinline__ uint32_t wave_in_block() {
  return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

__device__ __forceinline__ uint64_t wave_excl64(uint64_t x, int lane) {
  uint64_t incl = x;
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = uint64_t(__shfl_up(static_cast<unsigned long long>(incl), o));
    if (lane >= o) incl += y;
  }
  return incl - x;
}

// What lane c knows of column c of one sample after the parse.
struct Parsed {
  int status;    // MDSX_SAMPLE_* (wave-uniform), or MDSX_E_BOUNDS: the sample is not in the buffer
  int column;    // the column the status names (wave-uniform; -1: none)
  uint64_t src;  // the slice's first byte, from the sample's first
  uint64_t len;  // its clipped length
};

// mdsx_decode_sample's slicing (decode_sample_kernel) of the sample at data[0, n). Every lane of
// the wave takes part.
__device__ __forceinline__ Parsed parse_sample(const SamplesPlan& p, const uint8_t* data,
                                               uint64_t n, int lane) {
  Parsed r;
  r.column = -1, r.src = 0, r.len = 0;
  const bool col = lane < p.ncols;
  const int vi = col ? p.var_index[lane] : -1;
  // the heads: data[4 vi : 4 vi + 4] (mds/reader.py:118)
  const bool short_head = vi >= 0 && 4ull * uint64_t(vi) + 4 > n;
  const uint64_t sm = __ballot(short_head);
  if (sm) {  // numpy raises at the first head (column order) cut short
    r.status = MDSX_SAMPLE_SHORT_HEAD;
    r.column = __builtin_ctzll(sm);
    return r;
  }
  const uint64_t fixed = col ? uint64_t(p.row_bytes[lane]) : 0;
  const uint64_t size = vi >= 0 ? uint64_t(load_u32_any(data + 4u * uint32_t(vi))) : fixed;
  // column starts: 4 x nvar + the sizes before (mds/reader.py:122-125), then the slice's clip
  const uint64_t start = 4ull * uint64_t(p.nvar) + wave_excl64(size, lane);
  const uint64_t s = start < n ? start : n;
  const uint64_t e = start + size < n ? start + size : n;
  r.src = s;
  r.len = e - s;
  const uint64_t fm = __ballot(col && vi < 0 && r.len < size);
  const uint64_t cm = __ballot(vi >= 0 && r.len < size);
  r.status = fm ? MDSX_SAMPLE_SHORT_FIXED : cm ? MDSX_SAMPLE_CLIPPED : MDSX_SAMPLE_OK;
  if (fm) r.column = __builtin_ctzll(fm);
  else if (cm) r.column = __builtin_ctzll(cm);
  return r;
}

// Sample k of the table, checked against the buffer (with its slack on both sides).
__device__ __forceinline__ bool sample_span(const SamplesIn& in, uint64_t k, uint64_t* off,
                                            uint64_t* n) {
  *off = uniform64(in.offsets[k]);
  *n = uniform64(uint64_t(in.bytes[k]));
  return *off >= kSampleSlack && *off <= in.data_bytes && *n <= in.data_bytes - *off &&
         in.data_bytes - *off - *n >= kSampleSlack;
}

__global__ __launch_bounds__(64 * kSampleWaves) void samples_sizes_kernel(const SizesArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t k = uint64_t(blockIdx.x) * kSampleWaves + wave_in_block();
  if (k >= a.in.m) return;  // (the whole wave)
  uint64_t off, n;
  Parsed r;
  if (sample_span(a.in, k, &off, &n)) {
    r = parse_sample(a.plan, a.in.data + off, n, lane);
  } else {
    r.status = MDSX_E_BOUNDS, r.column = -1, r.src = 0, r.len = 0;
  }
  const int vi = lane < a.plan.ncols ? a.plan.var_index[lane] : -1;
  if (vi >= 0) a.lengths[uint64_t(vi) * (a.in.m + 1) + k + 1] = int64_t(r.len);
  if (lane == 0) {
    a.status[2 * k] = r.status;
    a.status[2 * k + 1] = r.column;
  }
}

__global__ __launch_bounds__(64 * kSampleWaves) void samples_copy_kernel(const CopyArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t k = uint64_t(blockIdx.x) * kSampleWaves + wave_in_block();
  if (k >= a.in.m) return;  // (the whole wave)
  uint64_t off, n;
  if (!sample_span(a.in, k, &off, &n)) return;
  const uint8_t* data = a.in.data + off;
  const Parsed r = parse_sample(a.plan, data, n, lane);
  if (r.status == MDSX_SAMPLE_SHORT_HEAD) return;  // every ragged length is 0, fixed rows stay 0
  const bool fixed_whole = r.status != MDSX_SAMPLE_SHORT_FIXED;
  for (int c = 0; c < a.plan.ncols; ++c) {  // uniform
    const uint64_t src = uniform64(uint64_t(__shfl(static_cast<unsigned long long>(r.src), c)));
    uint64_t len = uniform64(uint64_t(__shfl(static_cast<unsigned long long>(r.len), c)));
    if (a.plan.var_index[c] < 0) {
      // a whole fixed column to row k (a sample with a short one leaves all of them zero)
      if (fixed_whole && len && a.out[c])
        wave_copy<false, 2, false>(data + src, a.out[c] + k * uint64_t(a.plan.row_bytes[c]), len,
                                   lane);
      continue;
    }
    // the slice's place: [offsets[k], offsets[k + 1]) of the column's values, never more
    const int64_t o0 = int64_t(uniform64(uint64_t(a.offsets[c][k])));
    const int64_t o1 = int64_t(uniform64(uint64_t(a.offsets[c][k + 1])));
    if (o0 < 0 || o1 < o0 || uint64_t(o1) > a.capacity[c]) continue;
    if (uint64_t(o1 - o0) < len) len = uint64_t(o1 - o0);
    bool bad = false;
    if (len) {
      if (a.plan.kind[c] == MDSX_KIND_STR)
        bad = wave_copy<true, 2, false>(data + src, a.out[c] + o0, len, lane);
      else
        wave_copy<false, 2, false>(data + src, a.out[c] + o0, len, lane);
    }
    if (a.plan.kind[c] == MDSX_KIND_STR && a.flags[c] && lane == 0) a.flags[c][k] = bad ? 1 : 0;
  }
}

void fill_plan(const mdsx_plan* plan, SamplesPlan* p) {
  p->ncols = plan->ncols;
  p->nvar = plan->nvar;
  for (int c = 0; c < MDSX_MAX_COLUMNS; ++c) {
    const bool on = c < plan->ncols;
    p->row_bytes[c] = on ? uint32_t(plan->cols[c].row_bytes) : 0;
    p->var_index[c] = on ? int8_t(plan->cols[c].var_index) : int8_t(-1);
    p->kind[c] = on ? int8_t(plan->cols[c].kind) : int8_t(MDSX_KIND_FIXED);
  }
}

int fill_in(const char* who, const uint8_t* d_data, uint64_t data_bytes,
            const uint64_t* d_sample_offsets, const uint32_t* d_sample_bytes, uint64_t m,
            SamplesIn* in) {
  if (!d_data || !d_sample_offsets || !d_sample_bytes || m == 0 ||
      m > (uint64_t(1) << 31) || data_bytes < 2 * kSampleSlack)
    return mdsx::fail(MDSX_E_ARG, std::string(who) + ": null or empty argument");
  in->data = d_data;
  in->data_bytes = data_bytes;
  in->offsets = d_sample_offsets;
  in->bytes = d_sample_bytes;
  in->m = m;
  return MDSX_OK;
}

}  // namespace
}  // namespace mdsx_kernels

using namespace mdsx_kernels;

extern "C" {

int mdsx_decode_samples_sizes(const mdsx_plan* plan, const uint8_t* d_data, uint64_t data_bytes,
                              const uint64_t* d_sample_offsets, const uint32_t* d_sample_bytes,
                              uint64_t m, int64_t* d_lengths, int32_t* d_status, void* stream) {
  if (!plan || !d_status || (plan->nvar > 0 && !d_lengths))
    return mdsx::fail(MDSX_E_ARG, "mdsx_decode_samples_sizes: null argument");
  SizesArgs a;
  if (int rc = fill_in("mdsx_decode_samples_sizes", d_data, data_bytes, d_sample_offsets,
                       d_sample_bytes, m, &a.in))
    return rc;
  fill_plan(plan, &a.plan);
  a.lengths = d_lengths;
  a.status = d_status;
  const uint32_t blocks = uint32_t((m + kSampleWaves - 1) / kSampleWaves);
  hipLaunchKernelGGL(samples_sizes_kernel, dim3(blocks), dim3(64 * kSampleWaves), 0,
                     static_cast<hipStream_t>(stream), a);
  return hip_check(hipGetLastError(), "samples_sizes_kernel launch");
}

int mdsx_decode_samples_copy(const mdsx_plan* plan, const uint8_t* d_data, uint64_t data_bytes,
                             const uint64_t* d_sample_offsets, const uint32_t* d_sample_bytes,
                             uint64_t m, const mdsx_column_out* outs, void* stream) {
  if (!plan || !outs) return mdsx::fail(MDSX_E_ARG, "mdsx_decode_samples_copy: null argument");
  CopyArgs a;
  if (int rc = fill_in("mdsx_decode_samples_copy", d_data, data_bytes, d_sample_offsets,
                       d_sample_bytes, m, &a.in))
    return rc;
  fill_plan(plan, &a.plan);
  for (int c = 0; c < MDSX_MAX_COLUMNS; ++c) {
    const bool on = c < plan->ncols;
    const bool var = on && plan->cols[c].var_index >= 0;
    a.out[c] = on ? static_cast<uint8_t*>(outs[c].data) : nullptr;
    a.offsets[c] = var ? static_cast<const int64_t*>(outs[c].offsets) : nullptr;
    a.flags[c] = var ? static_cast<uint8_t*>(outs[c].flags) : nullptr;
    a.capacity[c] = var ? outs[c].capacity : 0;
    if (var && !a.offsets[c])
      return mdsx::fail(MDSX_E_ARG, "mdsx_decode_samples_copy: a ragged column without offsets");
    if (var && !a.out[c]) a.capacity[c] = 0;  // (nothing to write: every slice must be empty)
    if (on && !var && !a.out[c])
      return mdsx::fail(MDSX_E_ARG, "mdsx_decode_samples_copy: a fixed column without output");
  }
  const uint32_t blocks = uint32_t((m + kSampleWaves - 1) / kSampleWaves);
  hipLaunchKernelGGL(samples_copy_kernel, dim3(blocks), dim3(64 * kSampleWaves), 0,
                     static_cast<hipStream_t>(stream), a);
  return hip_check(hipGetLastError(), "samples_copy_kernel launch");
}

}  // extern "C"
