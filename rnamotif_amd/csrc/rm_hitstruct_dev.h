// rm_hitstruct_dev.h -- hit records expanded into per-base tensors on the device (rma_hit_structures, rm_hitpost.cpp):
// letter, element and mates of every base of every record's window.  The rule is rm_hitstruct.h's, shared with the host;
// spans, sources and offsets come from rm_hitwin_dev.hip (rma_hit_span_kernel, the exclusive scan).
//
//   rma_hit_helix_kernel    one lane per record: the one check rma_hit_span_kernel does not make -- the strands of a
//                           helix have one length -- a failing record's index into *bad by an atomic minimum
//   rma_hit_struct_kernel   one wave per record.  The record's offsets and lengths are read once, lane e holding element
//                           e and element 64 + e (two lane passes cover the 100 elements and 2 contexts a record can
//                           have); the program's table (HitStructTable) and the letters are read once per workgroup into
//                           LDS.  The lanes then take consecutive bases of the window, 64 at a time: a lane finds its
//                           element by walking the record's registers (wave-uniform lane reads, no memory), takes its
//                           helix from the table in LDS and the other strands' offsets from the lanes that hold them.
//                           base (1 byte) and elem (2 bytes) go out lane by lane, one contiguous run per wave.  mate is
//                           12 bytes a base, interleaved [T][3] as a consumer indexes it: the three words of a lane are
//                           handed round the wave (three rounds of lane shuffles, a 64 x 3 tile in registers) so that
//                           each of three store instructions writes 64 consecutive dwords -- 256 contiguous bytes, the
//                           coalesced form -- instead of 64 dwords 12 bytes apart.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_hitstruct.h"

namespace rma {

// Enqueue on s: *d_bad = min( *d_bad, h ) for every record h of [0, n) whose helices have strands of unequal length.
// d_table: the program's HitStructTable in device memory.  The records have passed hit_spans or are about to: only
// their length words are read.
hipError_t	hit_helix_check( const int32_t *d_hits, int64_t n, int stride, const HitStructTable *d_table, unsigned long long *d_bad,
	hipStream_t s );

// Enqueue on s: *d_carry += *d_add (one chunk's window bytes onto the running total)
hipError_t	hit_carry_add( int64_t *d_carry, const int64_t *d_add, hipStream_t s );

// what the fill kernel writes: record h's window at [ off[ h ], off[ h + 1 ] ) of base / elem / mate
struct HitStructOut {
	int64_t	*off;		// [ n + 1 ] of this chunk, n + 1 written only with `last`
	int32_t	*lo;		// [ n ]
	uint8_t	*base;		// the call's, indexed by off
	int16_t	*elem;
	int32_t	*mate;		// [ ][ 3 ]
};

// Enqueue on s: records [0, n) at d_hits, all checked, their lo / src (hit_spans) and offsets within the chunk d_offc
// (hit_offsets, d_offc[ 0 ] = 0), *d_carry the window bytes of the chunks before this one.  table / codes as hit_gather.
hipError_t	hit_struct_fill( const uint8_t *text, const int32_t *d_hits, int64_t n, int stride, const HitWinShape &shape,
	const HitStructTable *d_table, const int32_t *d_lo, const int64_t *d_src, const int64_t *d_offc, const int64_t *d_carry,
	const uint8_t *table, int codes, const HitStructOut &out, bool last, hipStream_t s );

}	// namespace rma
