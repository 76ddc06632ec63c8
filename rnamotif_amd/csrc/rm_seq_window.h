// rm_seq_window.h -- the base codes of a window of one strand of a packed entry, in one fetch.
//
// The packed database keeps 16 bases a dword in codes[] (2 bits each) and 32 a dword in amask[]
// (1: a letter that is not acgt), an entry's first base at a multiple of 32 (rm_pack.cpp).
// rmw_window_codes() turns strand positions [ p, p + n ) of the entry at off, slen bases long, strand comp, into
// what db_strand_code() gives base by base: 0..3, RMA_BC_N under the mask, the complement on strand 1 (whose
// position q is forward base slen - 1 - q).  It loads the dwords that hold a base of the window -- at most
// RMW_AWORDS of amask and RMW_CWORDS of codes for n <= RMW_MAX -- as independent loads ahead of any use, and
// nothing before the first or past the last of them: a word beyond the window's last is the last one read again.
//
// Plain C++ like rm_efn_core.h: the energy kernel's DevSeq uses it, and tests/hostsim compiles it for the CPU.
#pragma once
#include <stdint.h>
#include "rm_dev_program.h"

#ifndef RMD_FN
#define RMD_FN	static inline
#endif

#define RMW_MAX		96				// bases a window may have
#define RMW_AWORDS	( ( 31 + RMW_MAX + 31 ) / 32 )	// 4
#define RMW_CWORDS	( ( 15 + RMW_MAX + 15 ) / 16 )	// 7

RMD_FN void rmw_window_codes( const uint32_t *codes, const uint32_t *amask, int64_t off, int slen, int comp, int p, int n, uint8_t *out )
{
	const int64_t	f0 = off + ( comp ? slen - p - n : p ), f1 = f0 + n - 1;	// forward bases f0 .. f1
	const int64_t	a0 = f0 >> 5, c0 = f0 >> 4;
	const int	na = int( ( f1 >> 5 ) - a0 ), nc = int( ( f1 >> 4 ) - c0 );	// last word of each kind
	uint32_t	am[ RMW_AWORDS ], cw[ RMW_CWORDS ];
#pragma unroll
	for( int k = 0; k < RMW_AWORDS; k++ )
		am[ k ] = amask[ a0 + ( k < na ? k : na ) ];
#pragma unroll
	for( int k = 0; k < RMW_CWORDS; k++ )
		cw[ k ] = codes[ c0 + ( k < nc ? k : nc ) ];
	const int	odd = int( c0 & 1 );
	// word by word, so that the registers are named at compile time; a word's bases in a loop of at most 16 rounds
#pragma unroll
	for( int k = 0; k < RMW_CWORDS; k++ ){
		if( k > nc )
			break;
		const uint32_t	w = cw[ k ];
		// the 16 mask bits that go with codes word c0 + k
		static_assert( RMW_CWORDS >> 1 < RMW_AWORDS, "an odd first codes word" );
		const uint32_t	mw = odd ? am[ ( k + 1 ) >> 1 ] : am[ k >> 1 ];
		const uint32_t	m = ( ( odd + k ) & 1 ) ? mw >> 16 : mw & 0xffffu;
		const int64_t	b0 = ( c0 + k ) << 4;
		const int	lo = k == 0 ? int( f0 - b0 ) : 0, hi = k == nc ? int( f1 - b0 ) : 15;
#ifdef __clang__
#pragma clang loop vectorize( disable ) unroll( disable )	// (byte stores of a lane: nothing to gain, registers to lose)
#endif
		for( int r = lo; r <= hi; r++ ){
			const int	j = int( b0 - f0 ) + r;		// forward index in the window
			int	c = ( w >> ( 2 * r ) ) & 3;
			if( comp )
				c = 3 - c;
			if( ( m >> r ) & 1 )
				c = RMA_BC_N;
			out[ comp ? n - 1 - j : j ] = uint8_t( c );
		}
	}
}
