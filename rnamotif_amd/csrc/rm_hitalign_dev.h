// rm_hitalign_dev.h -- hit records laid into the columns of an alignment on the device (rma_hit_alignment_shape,
// rma_hit_alignment, rm_hitpost.cpp).  The rule is rm_hitalign.h's, shared with the host; the record check is
// rma_hit_span_kernel's (rm_hitwin_dev.hip), run before either kernel.
//
//   rma_hit_widths_kernel  a wave takes records in turn, lane e holding columns e and 64 + e -- two registers cover
//                          the 102 columns a descriptor can have -- and keeps the running maximum of the field widths
//                          in them.  The workgroup's waves combine in LDS (an atomic maximum there), then the
//                          workgroup issues one atomicMax per column into the call's 102 words.  Reads only the
//                          records' length words.
//   rma_hit_align_kernel   a wave per record.  The layout (column offsets, widths, directions: about 1.3 KB) and the
//                          letters are read once per workgroup into LDS; the record's offsets and lengths once into
//                          registers, lane e holding element e and element 64 + e as in rma_hit_struct_kernel.  The
//                          lanes then take 64 consecutive bytes of the row at a time: a lane finds its column in the
//                          table in LDS (hitalign_find_col), takes the element's offset and length from the lane that
//                          holds them, and hitalign_place() says whether its byte is a separator, gap, dot or letter.
//                          For a letter it fetches the text byte through hitwin_src and translates or complements
//                          it.  Each pass stores one contiguous run of 64 bytes of rows and, where asked for, 64
//                          consecutive dwords of pos.  rows is [ n ][ W ], indexed in 64 bits.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_hitalign.h"

namespace rma {

// Enqueue on s: d_widths[ c ] = max( d_widths[ c ], the width of column c's field in record h ) over records [0, n) at
// d_hits, c < hitalign_n_cols( shape ); d_widths: HA_MAX_COLS words the caller has set (to 0 for a new maximum).
hipError_t	hit_align_widths( const int32_t *d_hits, int64_t n, int stride, const HitWinShape &shape, int32_t *d_widths, hipStream_t s );

// Enqueue on s: rows [0, n) of d_rows (and of d_pos unless it is null) from records [0, n) at d_hits, all checked by
// hit_spans, every field no wider than its column in `lay`.  text, d_slen, d_start: the database's; table / codes as
// hit_gather.
hipError_t	hit_align_fill( const uint8_t *text, const int32_t *d_hits, int64_t n, int stride, const HitWinShape &shape,
	const HitAlignLayout &lay, const int32_t *d_slen, const int64_t *d_start, const uint8_t *table, int codes, uint8_t *d_rows,
	int32_t *d_pos, hipStream_t s );

}	// namespace rma
