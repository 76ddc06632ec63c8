// rm_hitwin.h -- the window of a hit record: what the score program and print_match() read of its strand.
//
// One rule for the host (Replayer::replay_packed, the replay of device databases) and the device (the span and
// gather kernels of rm_hitwin_dev.hip): the span is the least offset to the greatest end over the elements and,
// when the descriptor has them, the contexts, counting only those of positive length.  The letters of a window
// are the text's bytes as the readers deliver them (dbutil.c:112-113: a letter in lower case, u as t; here
// every other byte is n), on strand 1 the reverse complement mk_rcmp() makes of them (rnamot.c:193-216).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include "rnamotif_amd_program.h"

#if defined( __HIPCC__ )
#define RMW_FN	__host__ __device__ inline
#else
#define RMW_FN	inline
#endif

namespace rma {

// the readers' letter of a text byte
RMW_FN unsigned char hitwin_reader_letter( unsigned char b )
{
	if( b >= 'A' && b <= 'Z' )
		b = static_cast<unsigned char>( b + ( 'a' - 'A' ) );
	if( b >= 'a' && b <= 'z' )
		return b == 'u' ? 't' : b;
	return 'n';
}

// the letter of a code of a database's table (0-3; anything else is ambiguous)
RMW_FN unsigned char hitwin_code_letter( unsigned code )
{
	return code == 0 ? 'a' : code == 1 ? 'c' : code == 2 ? 'g' : code == 3 ? 't' : 'n';
}

// mk_rcmp's wc_cmp[]
RMW_FN unsigned char hitwin_wc_cmp( unsigned char c )
{
	switch( c ){
	case 'a' : case 'A' : return 't';
	case 'c' : case 'C' : return 'g';
	case 'g' : case 'G' : return 'c';
	case 't' : case 'T' : case 'u' : case 'U' : return 'a';
	default : return 'n';
	}
}

// what a record's window needs of the program
struct HitWinShape {
	int32_t	n_elems, ctx_off, has_lctx, has_rctx;
};

inline HitWinShape hitwin_shape( const rma_program_t &p )
{
	return HitWinShape{ p.n_elems, rma_hit_ctx_off( &p ), p.has_lctx, p.has_rctx };
}

enum { HW_OK = 0, HW_ENTRY, HW_STRAND, HW_EXTENT };

// The span [*lo, *hi) of record w (empty when *lo >= *hi: nothing of positive length), the record checked first:
// its entry inside [0, n_seq), its strand 0 or 1, every element and present context inside the entry's slen
// bases (off >= 0, len >= 0, off + len <= slen, summed in 64 bits).  Returns HW_OK or the first failing check,
// *which the element for HW_EXTENT (n_elems: the left context, n_elems + 1: the right one).  slen[] is read for
// an entry inside [0, n_seq) only.
RMW_FN int hitwin_span( const int32_t *w, const HitWinShape &s, int32_t n_seq, const int32_t *slen, int32_t *lo, int32_t *hi,
	int *which )
{
	*lo = 0;
	*hi = 0;
	*which = -1;
	const int32_t	seq = w[ 0 ], comp = w[ 1 ];
	if( seq < 0 || seq >= n_seq )
		return HW_ENTRY;
	if( comp != 0 && comp != 1 )
		return HW_STRAND;
	const int64_t	n = slen[ seq ];
	int64_t	l = n, h = 0;
	for( int e = 0; e < s.n_elems + 2; e++ ){
		int	k;
		if( e < s.n_elems )
			k = RMA_HIT_HDR + 4 * e;
		else if( e == s.n_elems && s.has_lctx )
			k = s.ctx_off;
		else if( e == s.n_elems + 1 && s.has_rctx )
			k = s.ctx_off + 2;
		else
			continue;
		const int64_t	off = w[ k ], len = w[ k + 1 ];
		if( off < 0 || len < 0 || off + len > n ){
			*which = e;
			return HW_EXTENT;
		}
		if( len > 0 ){
			l = off < l ? off : l;
			h = off + len > h ? off + len : h;
		}
	}
	*lo = static_cast<int32_t>( l );
	*hi = static_cast<int32_t>( h );
	return HW_OK;
}

// the length of a window (0 for an empty span)
RMW_FN int64_t hitwin_len( int32_t lo, int32_t hi )
{
	return hi > lo ? int64_t( hi ) - lo : 0;
}

// byte i of the window of a record on strand comp of an entry of slen bases whose span starts at lo: the
// entry's text byte it comes from (strand 1: counted from the 3' end, the byte's letter then complemented)
RMW_FN int64_t hitwin_src( int comp, int32_t slen, int32_t lo, int64_t i )
{
	return comp ? int64_t( slen ) - 1 - ( lo + i ) : lo + i;
}

// ---- the device half of rma_replay_device() (rm_hitpost.cpp) as the host half (rm_capi.cpp) sees it

// the device and page-locked buffers of one replay handle, made on its first use, on the database's device
struct HitWindowScratch;
void	hitwin_scratch_free( HitWindowScratch *s );

// A piece of a call's records with their windows, on the host: record h (0 <= h < n) is record first + h of the
// call, at records + h * stride; its window is windows[ off[ h ], off[ h + 1 ] ), the letters of positions
// [ lo[ h ], lo[ h ] + the window's length ) of its strand.  slen[ n_seq ]: the database's entry lengths.
struct HitWindowPiece {
	const int32_t	*records;
	int64_t	first, n;
	const char	*windows;
	const int64_t	*off;
	const int32_t	*lo;
	const int32_t	*slen;
	int32_t	n_seq;
};

}	// namespace rma

// The windows of the n_hits records at d_hits (device memory) of a database made by rma_db_create_device(), piece
// by piece in the order given, handed to `each` once every record has been checked on the device.  letters: 256
// bytes or null, as rma_replay_device() takes them.  Returns non-zero with err[] filled when something is refused
// or fails; an exception thrown by `each` passes through.
struct rma_db;
int	rma_hit_windows( rma::HitWindowScratch **scratch, const rma_db *db, const rma_program_t &prog, const int32_t *d_hits,
	int64_t n_hits, const uint8_t *letters, void *stream, const std::function<void( const rma::HitWindowPiece & )> &each,
	char *err, size_t errlen );
