// Stored beacon rows decoded on the device (check-chain ingest).
//
// ingest_row_decode restates the canonical-row rules of dgpu_ingest_decode
// (ingest.cpp, the yardstick: tests/ingest_rows_check.cpp compares the two
// field by field) as a host and device function:
//   {"PreviousSig":<hex or null>,"Round":<uint64>,"Signature":<hex or null>}
// in Go's field order, no whitespace; a field is null or a quoted even-length
// hex string of either letter case of at most `stride` bytes; Round is 1-20
// digits without a leading zero that fit 64 bits; the closing brace is the
// row's last byte.  A canonical row gives ok = 1 and both fields zero-padded
// to their strides; any other row ok = 0, round 0, both lengths 0 and both
// records zeroed.
//
// k_ingest_rows (one 64-lane wave per block, one row per lane) is a copy
// kernel with that parser in it: the wave copies its rows' byte range into
// LDS with 16-byte loads, every lane parses its own row there, decoding the
// hex in place (a decoded byte lands behind the read position), and the wave
// writes its 64 records, contiguous in each output array, with coalesced
// stores.  A wave whose rows are not an ascending disjoint run that fits the
// LDS budget, or that holds a row outside the buffer, parses straight from
// global memory, one row per lane.
//
// A host-only program includes this header under DG_NO_KERNELS and takes the
// parser alone.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef DG_FN
#define DG_FN __host__ __device__ __forceinline__
#endif

namespace dgpu {

// a canonical row is never longer than this at the given strides:
// {"PreviousSig":"..","Round":<20 digits>,"Signature":".."} = 64 + 2 (sig_stride + prev_stride)
DG_FN constexpr size_t ingest_row_max_len(size_t sig_stride, size_t prev_stride) {
  return 64 + 2 * (sig_stride + prev_stride);
}

// hex digit value, -1 for any other byte
DG_FN int ingest_hex(uint8_t c) {
  if (c >= '0' && c <= '9') return c - '0';
  const uint8_t l = (uint8_t)(c | 0x20);
  return (l >= 'a' && l <= 'f') ? l - 'a' + 10 : -1;
}

// the literal s at p (p advanced), or false.  Every byte is compared before
// the verdict: the loads do not wait for one another.
template <uint32_t N>
DG_FN bool ingest_lit(const uint8_t*& p, const uint8_t* end, const char (&s)[N]) {
  if ((size_t)(end - p) < N - 1) return false;
  uint32_t diff = 0;
  for (uint32_t k = 0; k + 1 < N; ++k) diff |= (uint32_t)(p[k] ^ (uint8_t)s[k]);
  if (diff) return false;
  p += N - 1;
  return true;
}
#define DG_INGEST_LIT(p, end, s) ingest_lit(p, end, s)

// "<hex>" or null -> out (at most stride bytes, no padding), *len; false = not
// canonical.  out may lie inside the row at or behind p (in-place decode): byte
// k is written after the two digits it comes from have been read.
DG_FN bool ingest_hex_field(const uint8_t*& p, const uint8_t* end, uint8_t* out, size_t stride, uint32_t* len) {
  if (DG_INGEST_LIT(p, end, "null")) {
    *len = 0;
    return true;
  }
  if (p >= end || *p != '"') return false;
  ++p;
  size_t k = 0;
  // eight bytes at a time while sixteen digits and room for them are left (the
  // loop below decides everything else): sixteen independent loads per step
  while (k + 8 <= stride && (size_t)(end - p) >= 16) {
    int v[16], any = 0;
    for (int j = 0; j < 16; ++j) any |= v[j] = ingest_hex(p[j]);
    if (any < 0) break;
    for (int j = 0; j < 8; ++j) out[k + j] = (uint8_t)(v[2 * j] << 4 | v[2 * j + 1]);
    k += 8;
    p += 16;
  }
  while (p + 1 < end) {
    const int a = ingest_hex(p[0]);
    if (a < 0) break;
    const int b = ingest_hex(p[1]);
    if (b < 0 || k == stride) return false;
    out[k++] = (uint8_t)(a << 4 | b);
    p += 2;
  }
  if (p >= end || *p != '"') return false;  // odd length, a non-hex byte, or no closing quote
  *len = (uint32_t)k;
  ++p;
  return true;
}

// The fields of one row: the decoded bytes alone (no padding; on false the
// outputs hold anything).  sig_out == nullptr is the in-place form: prev_out
// is the row itself and the signature's bytes follow the previous
// signature's (prev_out + *prev_len) -- both behind the parser's read
// position, inside the row's own bytes.
DG_FN bool ingest_row_fields(const uint8_t* row, uint32_t len, uint8_t* prev_out, size_t prev_stride, uint8_t* sig_out,
                             size_t sig_stride, uint64_t* round, uint32_t* prev_len, uint32_t* sig_len) {
  const uint8_t* p = row;
  const uint8_t* end = row + len;
  if (!DG_INGEST_LIT(p, end, "{\"PreviousSig\":") || !ingest_hex_field(p, end, prev_out, prev_stride, prev_len) ||
      !DG_INGEST_LIT(p, end, ",\"Round\":"))
    return false;
  const uint8_t* d = p;
  while (p < end && *p >= '0' && *p <= '9') ++p;
  const size_t nd = (size_t)(p - d);
  if (nd < 1 || nd > 20 || (nd > 1 && d[0] == '0')) return false;
  uint64_t r = 0;
  for (size_t k = 0; k < nd; ++k) {
    const uint64_t dig = (uint64_t)(d[k] - '0');
    if (r > (UINT64_MAX - dig) / 10) return false;
    r = r * 10 + dig;
  }
  *round = r;
  if (!sig_out) sig_out = prev_out + *prev_len;
  return DG_INGEST_LIT(p, end, ",\"Signature\":") && ingest_hex_field(p, end, sig_out, sig_stride, sig_len) &&
         DG_INGEST_LIT(p, end, "}") && p == end;
}

// dgpu_ingest_decode of one row: returns ok; the records are written in full
// (decoded bytes, then zeros to the stride; all zeros when not canonical).
DG_FN bool ingest_row_decode(const uint8_t* row, uint32_t len, uint64_t* round, uint8_t* sig, size_t sig_stride,
                             uint32_t* sig_len, uint8_t* prev, size_t prev_stride, uint32_t* prev_len) {
  uint64_t r = 0;
  uint32_t sl = 0, pl = 0;
  const bool g = ingest_row_fields(row, len, prev, prev_stride, sig, sig_stride, &r, &pl, &sl);
  if (!g) r = 0, sl = 0, pl = 0;
  for (size_t k = sl; k < sig_stride; ++k) sig[k] = 0;
  for (size_t k = pl; k < prev_stride; ++k) prev[k] = 0;
  *round = r;
  *sig_len = sl;
  *prev_len = pl;
  return g;
}

#ifndef DG_NO_KERNELS
// ---------------------------------------------------------------- kernel
constexpr int INGEST_ROWS_PER_WAVE = 64;
// LDS bytes of a wave's rows: 64 canonical rows at strides 96 / 96 (28,672
// bytes) and the up to 15 bytes that keep the copy's 16-byte phase; with the
// per-row words below a block stays under 32 KB, five blocks per CU
constexpr uint32_t INGEST_LDS_BYTES = 30720;
typedef uint32_t ingest_quad __attribute__((ext_vector_type(4)));  // one 16-byte load

// n fixed-stride records of one output array for the wave's cnt rows, from
// the rows' decoded bytes in LDS: record r = buf[at[r] .. at[r] + len[r]),
// zeros to the stride.  The wave's records are contiguous in out.
__device__ __forceinline__ void ingest_store_records(uint8_t* out, size_t stride, uint32_t cnt, const uint8_t* buf,
                                                     const uint32_t* at, const uint32_t* len, uint32_t lane) {
  const size_t total = (size_t)cnt * stride;
  if (!total) return;
  // element e (a word, or a byte) of the wave's records belongs to record e /
  // per at element e % per; a lane's elements are 64 apart: one division, then steps
  const bool words = stride % 4 == 0 && ((uintptr_t)out & 3) == 0;
  const uint32_t per = (uint32_t)(words ? stride / 4 : stride), count = (uint32_t)(words ? total / 4 : total);
  const uint32_t step_r = INGEST_ROWS_PER_WAVE / per, step_e = INGEST_ROWS_PER_WAVE % per;
  uint32_t r = lane / per, e = lane % per;
  for (uint32_t w = lane; w < count; w += INGEST_ROWS_PER_WAVE) {
    const uint32_t a = at[r], l = len[r];
    if (words) {
      const uint32_t b = e * 4;
      uint32_t v = 0;
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t)
        if (b + t < l) v |= (uint32_t)buf[a + b + t] << (8 * t);
      reinterpret_cast<uint32_t*>(out)[w] = v;
    } else {
      out[w] = e < l ? buf[a + e] : (uint8_t)0;
    }
    r += step_r, e += step_e;
    if (e >= per) e -= per, ++r;
  }
}

// Row i = row_len[i] bytes at rows + row_off[i] -> rounds[i], sigs + i *
// sig_stride (sig_len[i]), prev + i * prev_stride (prev_len[i]), ok[i]:
// dgpu_ingest_decode's outputs.  A row whose range leaves [0, rows_bytes) is
// not read (ok = 0).  Nothing outside [rows, rows + rows_bytes) is read: the
// copy into LDS takes 16-byte loads only between the first and the last
// 16-byte boundary inside the wave's range, single bytes before and after.
__global__ __launch_bounds__(INGEST_ROWS_PER_WAVE) void k_ingest_rows(
    size_t n, const uint8_t* __restrict__ rows, size_t rows_bytes, const uint64_t* __restrict__ row_off,
    const uint32_t* __restrict__ row_len, uint64_t* __restrict__ rounds, uint8_t* __restrict__ sigs, size_t sig_stride,
    uint32_t* __restrict__ sig_len, uint8_t* __restrict__ prev, size_t prev_stride, uint32_t* __restrict__ prev_len,
    uint8_t* __restrict__ ok) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[INGEST_LDS_BYTES];
  // where each row's decoded previous signature and signature lie in buf, and their lengths
  __shared__ uint32_t s_pa[INGEST_ROWS_PER_WAVE], s_sa[INGEST_ROWS_PER_WAVE], s_pl[INGEST_ROWS_PER_WAVE],
      s_sl[INGEST_ROWS_PER_WAVE];
  const uint32_t lane = threadIdx.x;
  const size_t i0 = (size_t)blockIdx.x * INGEST_ROWS_PER_WAVE;
  if (i0 >= n) return;
  const uint32_t cnt = (uint32_t)(n - i0 < (size_t)INGEST_ROWS_PER_WAVE ? n - i0 : (size_t)INGEST_ROWS_PER_WAVE);
  const size_t i = i0 + lane;
  const bool mine = lane < cnt;
  uint64_t off = 0;
  uint32_t len = 0;
  if (mine) off = row_off[i], len = row_len[i];
  const bool inside = off <= rows_bytes && len <= rows_bytes - off;
  // the wave's rows as one ascending run of disjoint ranges: row l starts at or after the end of row l - 1
  const unsigned long long end = off + len;  // (no wrap where `inside` holds)
  const unsigned long long prev_end = __shfl_up(end, 1);
  const bool in_order = lane == 0 || !mine || prev_end <= off;
  const uint64_t lo = __shfl((unsigned long long)off, 0), hi = __shfl(end, (int)cnt - 1);
  const bool staged = __all((!mine || inside) && in_order) && hi - lo + 15 <= INGEST_LDS_BYTES;
  if (!staged) {
    if (!mine) return;
    uint64_t r = 0;
    uint32_t sl = 0, pl = 0;
    uint8_t* so = sigs + i * sig_stride;
    uint8_t* po = prev + i * prev_stride;
    const bool g = ingest_row_decode(inside ? rows + off : rows, inside ? len : 0, &r, so, sig_stride, &sl, po,
                                     prev_stride, &pl);
    rounds[i] = r;
    sig_len[i] = sl;
    prev_len[i] = pl;
    ok[i] = g ? 1 : 0;
    return;
  }
  // [lo, hi) -> buf, keeping the bytes' position within a 16-byte line
  const uint8_t* src = rows + lo;
  const uint32_t span = (uint32_t)(hi - lo);
  const uint32_t ph = (uint32_t)((uintptr_t)src & 15);
  const uint32_t head = ph ? (16 - ph < span ? 16 - ph : span) : 0;
  const uint32_t quads = (span - head) / 16;
  const uint32_t tail = span - head - quads * 16;
  if (lane < head) buf[ph + lane] = src[lane];
  {
    const ingest_quad* q = reinterpret_cast<const ingest_quad*>(src + head);
    ingest_quad* b = reinterpret_cast<ingest_quad*>(buf + ((ph + head) & ~15u));
    // eight loads in flight per lane
    constexpr uint32_t U = 8;
    for (uint32_t k0 = lane; k0 < quads; k0 += U * INGEST_ROWS_PER_WAVE) {
      ingest_quad v[U];
#pragma unroll
      for (uint32_t j = 0; j < U; ++j)
        if (k0 + j * INGEST_ROWS_PER_WAVE < quads) v[j] = q[k0 + j * INGEST_ROWS_PER_WAVE];
#pragma unroll
      for (uint32_t j = 0; j < U; ++j)
        if (k0 + j * INGEST_ROWS_PER_WAVE < quads) b[k0 + j * INGEST_ROWS_PER_WAVE] = v[j];
    }
  }
  if (lane < tail) buf[ph + head + quads * 16 + lane] = src[head + quads * 16 + lane];
  __syncthreads();
  uint64_t r = 0;
  uint32_t sl = 0, pl = 0;
  bool g = false;
  if (mine) {
    uint8_t* row = buf + ph + (uint32_t)(off - lo);
    g = ingest_row_fields(row, len, row, prev_stride, nullptr, sig_stride, &r, &pl, &sl);
    if (!g) r = 0, sl = 0, pl = 0;
    s_pa[lane] = ph + (uint32_t)(off - lo);
    s_sa[lane] = s_pa[lane] + pl;  // the signature's bytes follow the previous signature's
    s_pl[lane] = pl;
    s_sl[lane] = sl;
    rounds[i] = r;
    sig_len[i] = sl;
    prev_len[i] = pl;
    ok[i] = g ? 1 : 0;
  }
  __syncthreads();
  ingest_store_records(prev + i0 * prev_stride, prev_stride, cnt, buf, s_pa, s_pl, lane);
  ingest_store_records(sigs + i0 * sig_stride, sig_stride, cnt, buf, s_sa, s_sl, lane);
}
#endif  // DG_NO_KERNELS

}  // namespace dgpu
