// Dense and packed typed batches from variable-length columns (gfx950): mdsx_ragged_elems,
// mdsx_ragged_pad, mdsx_ragged_pack.
//
// A decoded ragged column is packed bytes plus byte offsets; a dynamic ndarray row still starts
// with its header (NDArray.decode, encodings.py:270-305). These kernels turn such a column into
// what a model takes: dtype[rows, width] padded or cut to width (pad), or the rows' values back
// to back, aligned, with element offsets (pack, the cu_seqlens form). Both are byte movement plus
// optional integer widening; a row the reference's decode would refuse (status 1) or of another
// dtype than asked for (status 2) contributes no element.
//
// Work split. The grid covers destination bytes, not rows: a collate batch is a few hundred to a
// few thousand rows of 2-32 KiB, which a rows-per-workgroup mapping would put on a handful of
// CUs. A wave owns one kSegBytes segment of destination addresses (cut at 16-byte aligned
// addresses, so only a row's two ends have partial chunks): for pad, segment s of row r (a row
// has a fixed number of segments: width x item is the same for all); for pack, segment s of the
// packed output, whose rows it finds by binary search in the element offsets. Rows of less than
// kGroupBytes take the four-rows-per-wave form instead (one row per 16-lane group, group_copy),
// as the gather does.
//
// Ownership of destination bytes (neighbouring rows of a padded batch share 16-byte chunks
// whenever width x item is not a multiple of 16): a row's bytes are split into the data range
// and the pad range, the segment cuts both, and each piece is written by exactly one call --
// wave_copy / group_copy store whole aligned chunks only inside the piece and its partial end
// chunks one byte per lane; pad_fill does the same for the pad. No byte outside a row's
// [row start, row end) is written for that row, and no byte twice.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "mdsx_decode.h"
#include "mdsx_device.h"
#include "mdsx_internal.h"
#include "mdsx_ndarray.h"

namespace mdsx_kernels {

// mdsx_kernels.hip: exclusive scan of n tile totals (one workgroup); total -> dst_off[m].
__global__ void scan_tile_totals_kernel(const int64_t* in, int64_t* out, uint32_t n,
                                        int64_t* dst_off, uint64_t m, int64_t* out_total);

namespace {

// Destination bytes per wave: 8 KiB = two trips of wave_copy's 64 lanes x 4 chunks x 16 bytes.
// Enough to amortise a wave's row parse and (pack) its binary search; small enough that a
// 256-row batch of 32 KiB rows makes 1280 waves, more than the chip has SIMDs. Measured against
// 16 KiB: the same at 4096 rows within the spread, 16 % faster at 256 rows.
constexpr uint32_t kSegBytes = 8192;
// Destination rows (pad) or average rows (pack) under this many bytes: four rows per wave.
constexpr uint32_t kGroupBytes = 1024;
constexpr int kPackRowTile = 256;  // rows per workgroup of pack's scan and of its grouped copy
                                   // (the gather's tile: its workspace layout is reused)

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return uint64_t(uni(uint32_t(v))) | (uint64_t(uni(uint32_t(v >> 32))) << 32);
}

// The elements of row r: where its value bytes start, how many elements, and its status.
struct RowSpan {
  uint64_t src;
  int64_t n;
  uint32_t status;
};

__device__ __forceinline__ RowSpan row_span(const uint8_t* values, const int64_t* offsets,
                                            uint64_t r, int model, int src_id) {
  const int64_t b = offsets[r], len = offsets[r + 1] - b;
  RowSpan s{reinterpret_cast<uint64_t>(values) + uint64_t(b), 0, 0};
  if (model == MDSX_ROWS_PLAIN) {
    const int64_t item = src_id >> 3;
    if (len < 0 || (len & (item - 1))) s.status = 1;
    else s.n = len / item;
  } else {
    const NdRow h = ndarray_parse_row<false>(
        values + b, len, model == MDSX_ROWS_NDARRAY_STATIC ? src_id : 0, 0, nullptr);
    if (h.bad) s.status = 1;
    else if (h.id != uint32_t(src_id)) s.status = 2;
    else {
      s.n = h.numel;
      s.src += uint64_t(h.pos);
    }
  }
  return s;
}

// One source element of kS bytes at any byte address, sign- or zero-extended to 64 bits.
template <int kS, bool kSigned>
__device__ __forceinline__ uint64_t load_elem(uint64_t a, bool aligned) {
  uint64_t v;
  if (kS == 1) v = *gp_at<const uint8_t>(a);
  else if (aligned) v = kS == 2 ? uint64_t(*gp_at<const uint16_t>(a)) : uint64_t(*gp_at<const uint32_t>(a));
  else {
    v = 0;
#pragma unroll
    for (int b = 0; b < kS; ++b) v |= uint64_t(*gp_at<const uint8_t>(a + b)) << (8 * b);
  }
  if (kSigned) v = uint64_t(int64_t(v << (64 - 8 * kS)) >> (64 - 8 * kS));
  return v;
}

// n elements from src to dst, by one wave or (kGroup) by the 16-lane group of `lane`.
// kS == kD == 0: the same dtype, of `item` bytes: a bit copy (wave_copy / group_copy; clamped
// loads, the source is a caller's tensor; call under wave-uniform control flow with every lane
// active: they read across lanes; n is wave-uniform unless kGroup). Else integer widening from
// kS to kD bytes: dst is kD-aligned (a row of a kD-aligned tensor), src is not.
template <int kS, int kD, bool kSigned, bool kGroup>
__device__ __forceinline__ void row_copy(uint64_t src, uint64_t dst, uint64_t n, uint32_t item,
                                         int lane) {
  if constexpr (kS == kD) {
    if constexpr (kGroup)
      group_copy<2, true, true>(reinterpret_cast<const uint8_t*>(src),
                                reinterpret_cast<uint8_t*>(dst), n * item, lane);
    else if (n)
      wave_copy<false, 4, true, true, true>(reinterpret_cast<const uint8_t*>(src),
                                            reinterpret_cast<uint8_t*>(dst), n * item, lane);
  } else {
    constexpr int kLanes = kGroup ? 16 : 64;
    constexpr int kU = 4;  // loads in flight per lane
    const bool aligned = (src & (kS - 1)) == 0;
    for (uint64_t i0 = uint64_t(lane & (kLanes - 1)); i0 < n; i0 += kLanes * kU) {
      uint64_t v[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const uint64_t i = i0 + uint64_t(u) * kLanes;
        v[u] = i < n ? load_elem<kS, kSigned>(src + i * kS, aligned) : 0;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const uint64_t i = i0 + uint64_t(u) * kLanes;
        if (i >= n) break;
        if (kD == 4) __builtin_nontemporal_store(uint32_t(v[u]), gp_at<uint32_t>(dst + i * kD));
        else __builtin_nontemporal_store(v[u], gp_at<uint64_t>(dst + i * kD));
      }
    }
  }
}

// Fill [lo, hi) with the pad pattern (pat: the item's bytes repeated over 8 bytes; the byte at
// address A is byte A % 8 of it, the tensor being item-aligned): 16-byte stores for the aligned
// chunks wholly inside, one byte per lane for what is left at either end. l: the lane's index
// among the kLanes (>= 16) lanes that share the range.
template <int kLanes>
__device__ __forceinline__ void pad_fill(uint64_t lo, uint64_t hi, uint64_t pat, int l) {
  if (lo >= hi) return;
  const uint64_t a0 = (lo + 15) & ~uint64_t(15), a1 = hi & ~uint64_t(15);
  const uint4 v = make_uint4(uint32_t(pat), uint32_t(pat >> 32), uint32_t(pat), uint32_t(pat >> 32));
  if (a0 <= a1) {
    for (uint64_t a = a0 + 16 * uint64_t(l); a < a1; a += 16 * kLanes) st16<true>(a, v);
    if (l < 16) {
      const uint64_t A = lo + uint64_t(l), B = a1 + uint64_t(l);
      if (A < a0) *gp_at<uint8_t>(A) = uint8_t(pat >> (8 * (A & 7)));
      if (B < hi) *gp_at<uint8_t>(B) = uint8_t(pat >> (8 * (B & 7)));
    }
  } else if (l < 16) {  // inside one chunk
    const uint64_t A = lo + uint64_t(l);
    if (A < hi) *gp_at<uint8_t>(A) = uint8_t(pat >> (8 * (A & 7)));
  }
}

// Sizing pass: per-row element count and status; record = {max count, total count, rows with a
// non-zero status} (zeroed by the caller). One row per lane.
__global__ __launch_bounds__(kBlock) void ragged_elems_kernel(
    const uint8_t* values, const int64_t* offsets, uint64_t rows, int model, int src_id,
    int64_t* out_count, uint8_t* out_status, unsigned long long* record) {
  const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  uint64_t n = 0, bad = 0;
  if (r < rows) {
    const RowSpan s = row_span(values, offsets, r, model, src_id);
    n = uint64_t(s.n);
    bad = s.status ? 1 : 0;
    out_count[r] = s.n;
    out_status[r] = uint8_t(s.status);
  }
  uint64_t mx = n, sum = n;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, uint64_t(__shfl_xor(static_cast<unsigned long long>(mx), o)));
    sum += uint64_t(__shfl_xor(static_cast<unsigned long long>(sum), o));
    bad += uint64_t(__shfl_xor(static_cast<unsigned long long>(bad), o));
  }
  if ((threadIdx.x & 63) == 0) {
    if (mx) atomicMax(record, static_cast<unsigned long long>(mx));
    if (sum) atomicAdd(record + 1, static_cast<unsigned long long>(sum));
    if (bad) atomicAdd(record + 2, static_cast<unsigned long long>(bad));
  }
}

struct PadArgs {
  const uint8_t* values;
  const int64_t* offsets;
  uint64_t rows;
  uint64_t dst;        // address of dst[0, 0]
  uint64_t pat;        // the pad item repeated over 8 bytes
  int64_t* out_len;
  uint8_t* out_status;
  unsigned long long* bad_count;  // may be null
  uint32_t width;      // elements per destination row
  uint32_t row_bytes;  // width x destination item
  uint32_t sitem, ditem;
  uint32_t segs;       // segments per row (wave form)
  int32_t model, src_id;
  int32_t left, cut_left;
};

// What a row puts where in its destination row [R0, R0 + row_bytes).
struct PadPlan {
  uint64_t src;            // first source byte kept
  uint64_t d0, d1;         // data range (addresses)
  uint64_t p0, p1;         // pad range
  uint64_t kept;
};

__device__ __forceinline__ PadPlan pad_plan(const PadArgs& a, uint64_t row, uint64_t src,
                                            uint64_t n) {
  PadPlan p;
  p.kept = n < a.width ? n : uint64_t(a.width);
  const uint64_t skip = a.cut_left ? n - p.kept : 0;
  const uint64_t R0 = a.dst + row * a.row_bytes, R1 = R0 + a.row_bytes;
  p.src = src + skip * a.sitem;
  p.d0 = a.left ? R1 - p.kept * a.ditem : R0;
  p.d1 = p.d0 + p.kept * a.ditem;
  p.p0 = a.left ? R0 : p.d1;
  p.p1 = a.left ? p.d0 : R1;
  return p;
}

// dst[rows, width]: one launch, every byte of dst written once. Wave form: wave w takes segment
// w % segs of row w / segs. kGroup: 16 rows per workgroup, one per 16-lane group.
template <int kS, int kD, bool kSigned, bool kGroup>
__global__ __launch_bounds__(kBlock) void ragged_pad_kernel(const PadArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = uni(threadIdx.x >> 6);
  if constexpr (kGroup) {
    const uint64_t r0 = uint64_t(blockIdx.x) * (kBlock / 16) + wave * 4;
    if (r0 >= a.rows) return;  // wave-uniform
    const uint64_t row = r0 + uint64_t(lane >> 4);
    const bool live = row < a.rows;
    RowSpan s{0, 0, 0};
    if (live) s = row_span(a.values, a.offsets, row, a.model, a.src_id);
    const PadPlan p = pad_plan(a, live ? row : 0, s.src, uint64_t(s.n));
    row_copy<kS, kD, kSigned, true>(p.src, p.d0, live ? p.kept : 0, a.ditem, lane);
    if (live) {
      pad_fill<16>(p.p0, p.p1, a.pat, lane & 15);
      if ((lane & 15) == 0) {
        a.out_len[row] = int64_t(p.kept);
        a.out_status[row] = uint8_t(s.status);
        if (a.bad_count && s.status) atomicAdd(a.bad_count, 1ull);
      }
    }
  } else {
    const uint64_t w = uint64_t(blockIdx.x) * (kBlock / 64) + wave;
    const uint64_t row = w / a.segs;
    const uint32_t seg = uint32_t(w % a.segs);
    if (row >= a.rows) return;  // wave-uniform
    // every lane parses the same row: the results are made scalar, so what follows branches
    // with every lane active
    const RowSpan s = row_span(a.values, a.offsets, row, a.model, a.src_id);
    const uint32_t status = uni(s.status);
    const PadPlan p = pad_plan(a, row, uni64(s.src), uni64(uint64_t(s.n)));
    const uint64_t R0 = a.dst + row * a.row_bytes, R1 = R0 + a.row_bytes;
    const uint64_t A = (R0 & ~uint64_t(15)) + uint64_t(seg) * kSegBytes;
    const uint64_t S0 = max(R0, A), S1 = min(R1, A + kSegBytes);
    if (seg == 0 && lane == 0) {
      a.out_len[row] = int64_t(p.kept);
      a.out_status[row] = uint8_t(status);
      if (a.bad_count && status) atomicAdd(a.bad_count, 1ull);
    }
    if (S0 >= S1) return;  // the last segment of a row that starts on a chunk boundary
    const uint64_t lo = max(S0, p.d0), hi = min(S1, p.d1);
    if (lo < hi)  // cuts are chunk-aligned addresses: whole destination items
      row_copy<kS, kD, kSigned, false>(p.src + (lo - p.d0) / a.ditem * a.sitem, lo,
                                       (hi - lo) / a.ditem, a.ditem, lane);
    pad_fill<64>(max(S0, p.p0), min(S1, p.p1), a.pat, lane);
  }
}

// Pack, pass 1: tile-local exclusive scan of the counts and the tile totals.
__global__ __launch_bounds__(kBlock) void pack_scan_kernel(const int64_t* count, uint64_t rows,
                                                          int64_t* out_off, int64_t* tile_total) {
  __shared__ int64_t s_wsum[kBlock / 64];
  const uint64_t k = uint64_t(blockIdx.x) * kPackRowTile + threadIdx.x;
  const int64_t len = k < rows ? max(count[k], int64_t(0)) : 0;
  int64_t total;
  const int64_t excl = block_exclusive_scan(len, s_wsum, &total);
  if (k < rows) out_off[k] = excl;
  if (threadIdx.x == 0) tile_total[blockIdx.x] = total;
}

// Pack, pass 3 (after scan_tile_totals_kernel): final element offsets.
__global__ __launch_bounds__(kBlock) void pack_offsets_kernel(int64_t* out_off, uint64_t rows,
                                                             const int64_t* tile_prefix) {
  const uint64_t k = uint64_t(blockIdx.x) * kPackRowTile + threadIdx.x;
  if (k < rows) out_off[k] += tile_prefix[blockIdx.x];
}

struct PackArgs {
  const uint8_t* values;
  const int64_t* offsets;
  uint64_t rows;
  uint64_t dst;
  uint64_t capacity;  // elements
  const int64_t* off; // final element offsets [rows + 1]
  uint32_t sitem, ditem;
  int32_t model, src_id;
};

// A row is copied when it is good, its element count is what the offsets were built from, and
// it ends inside the destination.
__device__ __forceinline__ bool pack_row_ok(const PackArgs& a, const RowSpan& s, int64_t off,
                                            int64_t end) {
  return s.status == 0 && s.n == end - off && off >= 0 && end > off &&
         uint64_t(end) <= a.capacity;
}

// Pack, pass 4. Wave form: a wave takes one kSegBytes segment of the packed output and copies
// the part of every row that lies in it. kGroup: a workgroup takes kPackRowTile rows, four per
// wave step (gather_copy_kernel's form).
template <int kS, int kD, bool kSigned, bool kGroup>
__global__ __launch_bounds__(kBlock) void ragged_pack_kernel(const PackArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = uni(threadIdx.x >> 6);
  if constexpr (kGroup) {
    __shared__ uint64_t s_src[kPackRowTile];
    __shared__ int64_t s_dst[kPackRowTile];
    __shared__ int64_t s_n[kPackRowTile];
    const uint64_t k0 = uint64_t(blockIdx.x) * kPackRowTile;
    {
      const uint64_t k = k0 + threadIdx.x;
      int64_t n = 0;
      if (k < a.rows) {
        const RowSpan s = row_span(a.values, a.offsets, k, a.model, a.src_id);
        const int64_t off = a.off[k], end = a.off[k + 1];
        if (pack_row_ok(a, s, off, end)) n = s.n;
        s_src[threadIdx.x] = s.src;
        s_dst[threadIdx.x] = off;
      }
      s_n[threadIdx.x] = n;
    }
    __syncthreads();
    for (int r0 = int(wave) * 4; r0 < kPackRowTile; r0 += kBlock / 16) {
      if (k0 + r0 >= a.rows) break;  // wave-uniform
      const int i = r0 + (lane >> 4);
      const bool live = s_n[i] > 0;
      row_copy<kS, kD, kSigned, true>(live ? s_src[i] : a.dst,
                                      live ? a.dst + uint64_t(s_dst[i]) * a.ditem : a.dst,
                                      live ? uint64_t(s_n[i]) : 0, a.ditem, lane);
    }
  } else {
    const uint64_t w = uint64_t(blockIdx.x) * (kBlock / 64) + wave;
    const uint64_t total = min(uint64_t(max(a.off[a.rows], int64_t(0))), a.capacity);
    const uint64_t end_addr = a.dst + uni64(total) * a.ditem;
    const uint64_t A = (a.dst & ~uint64_t(15)) + w * kSegBytes;
    const uint64_t S0 = max(a.dst, A), S1 = min(end_addr, A + kSegBytes);
    if (S0 >= S1) return;  // wave-uniform
    // the first row that ends after the segment's first element
    const int64_t e0 = int64_t((S0 - a.dst) / a.ditem);
    uint64_t lo_r = 0, hi_r = a.rows;
    while (lo_r < hi_r) {
      const uint64_t mid = (lo_r + hi_r) >> 1;
      if (a.off[mid + 1] > e0) hi_r = mid;
      else lo_r = mid + 1;
    }
    for (uint64_t i = uni64(lo_r); i < a.rows; ++i) {
      const int64_t off = int64_t(uni64(uint64_t(a.off[i])));
      const int64_t end = int64_t(uni64(uint64_t(a.off[i + 1])));
      if (off < 0 || a.dst + uint64_t(off) * a.ditem >= S1) break;
      if (end <= off) continue;
      const RowSpan s = row_span(a.values, a.offsets, i, a.model, a.src_id);
      const RowSpan us{uni64(s.src), int64_t(uni64(uint64_t(s.n))), uni(s.status)};
      if (!pack_row_ok(a, us, off, end)) continue;
      const uint64_t d0 = a.dst + uint64_t(off) * a.ditem, d1 = a.dst + uint64_t(end) * a.ditem;
      const uint64_t lo = max(S0, d0), hi = min(S1, d1);
      if (lo < hi)
        row_copy<kS, kD, kSigned, false>(us.src + (lo - d0) / a.ditem * a.sitem, lo,
                                         (hi - lo) / a.ditem, a.ditem, lane);
    }
  }
}

template <int N>
using IntC = std::integral_constant<int, N>;

// Calls f(source item, destination item, signed) for an allowed conversion: equal dtypes (0, 0:
// a bit copy), int8/uint8/int16/uint16 -> int32/int64, int32/uint32 -> int64.
template <class F>
bool with_conversion(int src_id, int dst_id, F&& f) {
  if (src_id == dst_id) {
    f(IntC<0>{}, IntC<0>{}, std::false_type{});
    return true;
  }
  const bool src_int = src_id == 8 || src_id == 9 || src_id == 16 || src_id == 17 ||
                       src_id == 32 || src_id == 33;
  if (!src_int || !(dst_id == 33 || dst_id == 65)) return false;
  const int s = src_id >> 3, d = dst_id >> 3;
  if (s >= d) return false;
  const bool sgn = src_id & 1;
#define MDSX_CONV(S, D)                                   \
  if (s == S && d == D) {                                 \
    if (sgn) f(IntC<S>{}, IntC<D>{}, std::true_type{});   \
    else f(IntC<S>{}, IntC<D>{}, std::false_type{});      \
    return true;                                          \
  }
  MDSX_CONV(1, 4)
  MDSX_CONV(1, 8)
  MDSX_CONV(2, 4)
  MDSX_CONV(2, 8)
  MDSX_CONV(4, 8)
#undef MDSX_CONV
  return false;
}

bool conversion_ok(int src_id, int dst_id) {
  return with_conversion(src_id, dst_id, [](auto, auto, auto) {});
}

// The argument checks the three entry points share (before any HIP call).
int check_rows(const char* who, const uint8_t* values, const int64_t* offsets, uint64_t rows,
               int model, int src_id) {
  if (!offsets || (rows && !values) || rows >= (uint64_t(1) << 40))
    return mdsx::fail(MDSX_E_ARG, std::string(who) + ": bad argument");
  if (model != MDSX_ROWS_PLAIN && model != MDSX_ROWS_NDARRAY_STATIC &&
      model != MDSX_ROWS_NDARRAY_DYN)
    return mdsx::fail(MDSX_E_ARG, std::string(who) + ": unknown row model");
  if (!value_dtype_ok(uint32_t(src_id)))
    return mdsx::fail(MDSX_E_ENCODING, std::string(who) + ": unknown dtype id");
  return MDSX_OK;
}

}  // namespace
}  // namespace mdsx_kernels

using namespace mdsx_kernels;

extern "C" {

int mdsx_ragged_elems(const uint8_t* values, const int64_t* offsets, uint64_t rows, int row_model,
                      int src_dtype, int64_t* out_count, uint8_t* out_status, int64_t* d_record,
                      void* stream) {
  int rc = check_rows("mdsx_ragged_elems", values, offsets, rows, row_model, src_dtype);
  if (rc != MDSX_OK) return rc;
  if (!d_record || (rows && (!out_count || !out_status)))
    return mdsx::fail(MDSX_E_ARG, "mdsx_ragged_elems: bad argument");
  if (rows == 0) return MDSX_OK;
  const unsigned grid = unsigned((rows + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(ragged_elems_kernel, dim3(grid), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), values, offsets, rows, row_model, src_dtype,
                     out_count, out_status, reinterpret_cast<unsigned long long*>(d_record));
  return hip_check(hipGetLastError(), "ragged_elems_kernel launch");
}

int mdsx_ragged_pad(const uint8_t* values, const int64_t* offsets, uint64_t rows, int row_model,
                    int src_dtype, int dst_dtype, void* dst, uint64_t width, int side,
                    int truncate, uint64_t pad_bits, int64_t* out_len, uint8_t* out_status,
                    int64_t* d_bad_count, void* stream) {
  int rc = check_rows("mdsx_ragged_pad", values, offsets, rows, row_model, src_dtype);
  if (rc != MDSX_OK) return rc;
  if (!value_dtype_ok(uint32_t(dst_dtype)))
    return mdsx::fail(MDSX_E_ENCODING, "mdsx_ragged_pad: unknown dtype id");
  if (!conversion_ok(src_dtype, dst_dtype))
    return mdsx::fail(MDSX_E_ARG, "mdsx_ragged_pad: conversion not allowed (equal dtypes, or "
                                  "integer widening to int32 / int64)");
  const uint64_t ditem = uint64_t(dst_dtype >> 3);
  if (width == 0 || width >= (uint64_t(1) << 32) || width * ditem >= (uint64_t(1) << 32))
    return mdsx::fail(MDSX_E_ARG, "mdsx_ragged_pad: width x item must be in [1, 2^32)");
  if ((side != MDSX_SIDE_RIGHT && side != MDSX_SIDE_LEFT) ||
      (truncate != MDSX_SIDE_RIGHT && truncate != MDSX_SIDE_LEFT))
    return mdsx::fail(MDSX_E_ARG, "mdsx_ragged_pad: side / truncate must be MDSX_SIDE_*");
  if (rows && (!dst || !out_len || !out_status || (reinterpret_cast<uint64_t>(dst) & (ditem - 1))))
    return mdsx::fail(MDSX_E_ARG, "mdsx_ragged_pad: bad argument");
  if (rows == 0) return MDSX_OK;
  PadArgs a;
  a.values = values;
  a.offsets = offsets;
  a.rows = rows;
  a.dst = reinterpret_cast<uint64_t>(dst);
  uint64_t pat = ditem == 8 ? pad_bits : pad_bits & ((uint64_t(1) << (8 * ditem)) - 1);
  for (uint64_t b = ditem; b < 8; b *= 2) pat |= pat << (8 * b);
  a.pat = pat;
  a.out_len = out_len;
  a.out_status = out_status;
  a.bad_count = reinterpret_cast<unsigned long long*>(d_bad_count);
  a.width = uint32_t(width);
  a.row_bytes = uint32_t(width * ditem);
  a.sitem = uint32_t(src_dtype >> 3);
  a.ditem = uint32_t(ditem);
  // a row that does not start on a chunk boundary reaches into one more segment
  a.segs = (a.row_bytes + 15 + kSegBytes - 1) / kSegBytes;
  a.model = row_model;
  a.src_id = src_dtype;
  a.left = side == MDSX_SIDE_LEFT;
  a.cut_left = truncate == MDSX_SIDE_LEFT;
  const bool group = a.row_bytes < kGroupBytes;
  const uint64_t blocks = group ? (rows + kBlock / 16 - 1) / (kBlock / 16)
                                : (rows * a.segs + kBlock / 64 - 1) / (kBlock / 64);
  if (blocks >= (uint64_t(1) << 31))
    return mdsx::fail(MDSX_E_ARG, "mdsx_ragged_pad: batch too large for one launch");
  hipStream_t s = static_cast<hipStream_t>(stream);
  with_conversion(src_dtype, dst_dtype, [&](auto S, auto D, auto sgn) {
    constexpr int kS = decltype(S)::value, kD = decltype(D)::value;
    constexpr bool kSigned = decltype(sgn)::value;
    if (group)
      hipLaunchKernelGGL((ragged_pad_kernel<kS, kD, kSigned, true>), dim3(unsigned(blocks)),
                         dim3(kBlock), 0, s, a);
    else
      hipLaunchKernelGGL((ragged_pad_kernel<kS, kD, kSigned, false>), dim3(unsigned(blocks)),
                         dim3(kBlock), 0, s, a);
  });
  return hip_check(hipGetLastError(), "ragged_pad_kernel launch");
}

int mdsx_ragged_pack(const uint8_t* values, const int64_t* offsets, uint64_t rows, int row_model,
                     int src_dtype, int dst_dtype, const int64_t* d_count, void* dst,
                     uint64_t dst_capacity, int64_t* out_offsets, void* d_workspace,
                     uint64_t workspace_bytes, void* stream) {
  int rc = check_rows("mdsx_ragged_pack", values, offsets, rows, row_model, src_dtype);
  if (rc != MDSX_OK) return rc;
  if (!value_dtype_ok(uint32_t(dst_dtype)))
    return mdsx::fail(MDSX_E_ENCODING, "mdsx_ragged_pack: unknown dtype id");
  if (!conversion_ok(src_dtype, dst_dtype))
    return mdsx::fail(MDSX_E_ARG, "mdsx_ragged_pack: conversion not allowed (equal dtypes, or "
                                  "integer widening to int32 / int64)");
  const uint64_t ditem = uint64_t(dst_dtype >> 3);
  if (!out_offsets || (dst_capacity && !dst) || dst_capacity >= (uint64_t(1) << 56) ||
      (reinterpret_cast<uint64_t>(dst) & (ditem - 1)) ||
      (rows && (!d_count || !d_workspace || workspace_bytes < mdsx_gather_workspace_bytes(rows))))
    return mdsx::fail(MDSX_E_ARG, "mdsx_ragged_pack: bad argument");
  const uint64_t tiles = (rows + kPackRowTile - 1) / kPackRowTile;
  const bool group = dst_capacity * ditem < uint64_t(kGroupBytes) * rows;
  const uint64_t blocks =
      group ? tiles : ((dst_capacity * ditem + 15 + kSegBytes - 1) / kSegBytes + 3) / 4;
  if (blocks >= (uint64_t(1) << 31))
    return mdsx::fail(MDSX_E_ARG, "mdsx_ragged_pack: batch too large for one launch");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rows == 0)  // nothing launched; offsets[0] is the caller's (a one-element zero tensor)
    return MDSX_OK;
  // the gather's workspace layout: [256: status][tile totals][tile prefixes]
  uint8_t* wsb = static_cast<uint8_t*>(d_workspace);
  int64_t* tt = reinterpret_cast<int64_t*>(wsb + 256);
  int64_t* tp = reinterpret_cast<int64_t*>(wsb + 256 + ((tiles * 8 + 255) & ~uint64_t(255)));
  hipLaunchKernelGGL(pack_scan_kernel, dim3(unsigned(tiles)), dim3(kBlock), 0, s, d_count, rows,
                     out_offsets, tt);
  rc = hip_check(hipGetLastError(), "pack_scan_kernel launch");
  if (rc != MDSX_OK) return rc;
  hipLaunchKernelGGL(scan_tile_totals_kernel, dim3(1), dim3(kBlock), 0, s, tt, tp,
                     uint32_t(tiles), out_offsets, rows, static_cast<int64_t*>(nullptr));
  rc = hip_check(hipGetLastError(), "scan_tile_totals_kernel launch");
  if (rc != MDSX_OK) return rc;
  hipLaunchKernelGGL(pack_offsets_kernel, dim3(unsigned(tiles)), dim3(kBlock), 0, s, out_offsets,
                     rows, tp);
  rc = hip_check(hipGetLastError(), "pack_offsets_kernel launch");
  if (rc != MDSX_OK || dst_capacity == 0) return rc;
  PackArgs a;
  a.values = values;
  a.offsets = offsets;
  a.rows = rows;
  a.dst = reinterpret_cast<uint64_t>(dst);
  a.capacity = dst_capacity;
  a.off = out_offsets;
  a.sitem = uint32_t(src_dtype >> 3);
  a.ditem = uint32_t(ditem);
  a.model = row_model;
  a.src_id = src_dtype;
  with_conversion(src_dtype, dst_dtype, [&](auto S, auto D, auto sgn) {
    constexpr int kS = decltype(S)::value, kD = decltype(D)::value;
    constexpr bool kSigned = decltype(sgn)::value;
    if (group)
      hipLaunchKernelGGL((ragged_pack_kernel<kS, kD, kSigned, true>), dim3(unsigned(blocks)),
                         dim3(kBlock), 0, s, a);
    else
      hipLaunchKernelGGL((ragged_pack_kernel<kS, kD, kSigned, false>), dim3(unsigned(blocks)),
                         dim3(kBlock), 0, s, a);
  });
  return hip_check(hipGetLastError(), "ragged_pack_kernel launch");
}

}  // extern "C"
