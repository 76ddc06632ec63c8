// rm_hitpost.h -- where the arrays of rm_hitpost.cpp's scratch blocks lie.  In a header of their own so that a host
// program can hold them to the offsets written out by hand (tests/hostsim/carve_check.cpp).
#pragma once
#include "rm_scanner_impl.h"
#include "rm_prune_dev.h"

namespace rma {

// The words of a window scratch's `bad` arrays.  On the device a word holds the least index of a refused record, ~0
// for none; the kernels lower it with an atomic minimum.  Page-locked: what a call copies back for its one wait.
enum HitBadSlot {
	HB_RECORD,		// a bad record, by the span rule (and, for structures, the helix check): check_records resets it
	HB_STRUCT_SPARE,	// structures: where the spans of a chunk put theirs once every record has been judged
	HB_PRINT_TEXT,		// print: a text_len outside its row
	HB_PRINT_SPARE, HB_PRINT_TEXT_SPARE,	// print: where the fill call's second pass over the sizes puts the two
	HB_CT,			// .ct: the refused record and why, ( index << 4 ) | code
	HB_CT_SPARE,		// .ct: where the fill call's second pass over the sizes puts it
	HB_SLOTS
};
enum HitBadHostSlot {
	HBH_FIRST,		// the call's refusal word
	HBH_TOTAL,		// the running total (a sized call's bytes)
	HBH_SECOND,		// a sized call's second refusal word (print: HB_PRINT_TEXT)
	HBH_SLOTS
};
// (Carver::take gives every array 256 bytes at least: as long as the words fit, the arrays behind them stay where they are)
static_assert( HB_SLOTS * 8 <= 256 && HBH_SLOTS * 8 <= 256, "the refusal words outgrow their 256 bytes: the letters behind them move" );

// the two fixed blocks of a window scratch, for chunks of `chunk` records; carve_*: the block's size
struct HitWinFixed {
	// device: lo[ chunk ] | len[ chunk + 1 ] | off[ chunk + 1 ] | src[ chunk ] | bad[ HB_SLOTS ] | letters[ 256 ]
	// page-locked: off[ chunk + 1 ] | lo[ chunk ] | bad[ HBH_SLOTS ] | letters[ 256 ]
	int32_t	*d_lo = nullptr, *h_lo = nullptr;
	int64_t	*d_len = nullptr, *d_off = nullptr, *d_src = nullptr, *h_off = nullptr;
	unsigned long long	*d_bad = nullptr, *h_bad = nullptr;
	uint8_t	*d_tab = nullptr, *h_tab = nullptr;
	size_t	carve_dev( void *base, size_t chunk )
	{
		Carver	c;
		d_lo = c.take<int32_t>( base, chunk );
		d_len = c.take<int64_t>( base, chunk + 1 );
		d_off = c.take<int64_t>( base, chunk + 1 );
		d_src = c.take<int64_t>( base, chunk );
		d_bad = c.take<unsigned long long>( base, HB_SLOTS );
		d_tab = c.take<uint8_t>( base, 256 );
		return c.at;
	}
	size_t	carve_host( void *base, size_t chunk )
	{
		Carver	c;
		h_off = c.take<int64_t>( base, chunk + 1 );
		h_lo = c.take<int32_t>( base, chunk );
		h_bad = c.take<unsigned long long>( base, HBH_SLOTS );
		h_tab = c.take<uint8_t>( base, 256 );
		return c.at;
	}
};

// the block of one rma_prune_hits() call over n records of `row` key words each, in `parts` workgroups: its size
inline size_t prune_carve( PruneDev &pd, void *base, size_t n, size_t parts, size_t row )
{
	Carver	c;
	pd.hdr = c.take<int32_t>( base, n * 4 );
	pd.rows = c.take<int32_t>( base, n * row );
	pd.bflag = c.take<uint8_t>( base, n );
	pd.part = c.take<long long>( base, parts );
	pd.part_x = c.take<long long>( base, parts );
	pd.blocks = c.take<long long>( base, n );
	return c.at;
}

}	// namespace rma
