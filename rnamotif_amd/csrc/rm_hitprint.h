// rm_hitprint.h -- the printed form of a hit record: the two lines HitPrinter::print (rm_score.cpp:1909) puts on
// stdout for it, print_match() of the reference (find_motif.c:1869-1896), as bytes.
//
// One rule for the host (tests/hostsim/hit_print_check.cpp, the reasons rma_hit_print() gives for a refusal) and the
// device (the size and fill kernels of rm_hitprint_dev.hip).  For record w of a program, of an entry of slen bases
// named sid with the definition sdef, whose score column is the text_len bytes rma_score_hits_text() delivers
// (rm_score_fmt.h has written them: %8d, %8.3lf or %8s of the SCORE):
//
//   definition line   ">" sid " " sdef "\n"
//   hit line          %-12s of sid, a blank, the score column, " %d %7d %4d" of comp, offset and len, one field per
//                     printed element, "\n"
//   offset            comp ? slen - matchoff( descr[ 0 ] ) : matchoff( descr[ 0 ] ) + 1
//   len               the sum of the elements' matchlen, without the contexts
//   field             the left context when the descriptor has one, every element, the right context when it has one
//                     (the columns of rm_hitalign.h); " " and the element's letters, " ." where its length is 0
//   letters           rm_hitwin.h's: the reader's letter or the table's of the entry's text byte hitwin_src() names, on
//                     strand 1 complemented -- what rma_hit_gather_kernel reads
//   integers          rms_fmt_int of rm_score_fmt.h; the widths 7 and 4 are minimums, as in printf
//
// The lines are a row of segments (hitprint_seg): 10 fixed ones and one per field, at most 112.  hitprint_size() is the
// sum of their lengths in 64 bits and 0 for a record that is not to be printed; hitprint_seg_byte() gives byte j of a
// segment and hitprint_byte() byte b of the lines.  A record is checked by hitwin_span's checks, with its codes,
// before anything of it is used; its text_len must lie inside [0, text_width] (HP_TEXT).  The host printer cuts a sid
// of 2048 bytes or more (snprintf into buf[ 2048 ]); the rule does not restate that: such a name is refused where
// names are made (HP_MAX_SID).
#pragma once
#include "rm_hitalign.h"
#if defined( __HIPCC__ ) && !defined( RMD_FN )
#define RMD_FN		static __host__ __device__ inline
#define RMD_FN_MEMBER	__host__ __device__ inline
#endif
#include "rm_score_fmt.h"

namespace rma {

enum { HP_CONST = 0, HP_SID, HP_SDEF, HP_SCORE, HP_NUM, HP_FIELD };		// what a segment is
enum { HP_FIXED_SEGS = 10, HP_FIRST_FIELD = 9, HP_MAX_SEGS = HP_FIXED_SEGS + HA_MAX_COLS };
// " %d %7d %4d" of a checked record -- comp is 0 or 1, the other two any int -- has at most 2 + 12 + 12 = 26 bytes
enum { HP_SID_WIDTH = 12, HP_MAX_SID = 2047, HP_NUM_CAP = 32 };
enum { HP_TEXT = HS_HELIX + 1 };		// the record check's code for a text_len outside [0, text_width]

// what the lines of a record need beside its words
struct HitPrintIn {
	int64_t	sid_len, sdef_len;
	int32_t	slen;		// its entry's bases
	int32_t	text_len;	// its score column's bytes
};

// a segment: CONST `arg` len times; SID, SDEF, SCORE, NUM their bytes; FIELD: a blank, then the letters of the
// element whose offset is word `arg` of the record, or "."
struct HitPrintSeg {
	int32_t	kind, arg;
	int64_t	len;
};

// (the host's ints wrap where a record somebody made by hand overflows them)
RMW_FN int32_t hitprint_offset( const int32_t *w, int32_t slen )
{
	const uint32_t	off0 = uint32_t( w[ RMA_HIT_HDR ] );
	return int32_t( w[ 1 ] ? uint32_t( slen ) - off0 : off0 + 1u );
}

RMW_FN int32_t hitprint_len( const int32_t *w, const HitWinShape &s )
{
	uint32_t	n = 0;
	for( int e = 0; e < s.n_elems; e++ )
		n += uint32_t( w[ RMA_HIT_HDR + 4 * e + 1 ] );
	return int32_t( n );
}

// " %d %7d %4d" of comp, offset and len into buf[ cap ]; returns its length (cap 0: the length alone)
RMW_FN int hitprint_numbers( const int32_t *w, const HitWinShape &s, int32_t slen, uint8_t *buf, int cap )
{
	RmsSink	o{ buf, 1, 0, cap, 0 };
	o.put( ' ' );
	rms_fmt_int( o, RmsSpec{ 0, 0, -1 }, 'd', w[ 1 ] );
	o.put( ' ' );
	rms_fmt_int( o, RmsSpec{ 0, 7, -1 }, 'd', hitprint_offset( w, slen ) );
	o.put( ' ' );
	rms_fmt_int( o, RmsSpec{ 0, 4, -1 }, 'd', hitprint_len( w, s ) );
	return o.n;
}

RMW_FN int hitprint_n_segs( const HitWinShape &s )
{
	return HP_FIXED_SEGS + hitalign_n_cols( s );
}

// segment k (0 <= k < hitprint_n_segs) of a checked record's lines; num_len: what hitprint_numbers returned
RMW_FN HitPrintSeg hitprint_seg( const int32_t *w, const HitWinShape &s, const HitPrintIn &in, int num_len, int k )
{
	switch( k ){
	case 0 : return HitPrintSeg{ HP_CONST, '>', 1 };
	case 1 : return HitPrintSeg{ HP_SID, 0, in.sid_len };
	case 2 : return HitPrintSeg{ HP_CONST, ' ', 1 };
	case 3 : return HitPrintSeg{ HP_SDEF, 0, in.sdef_len };
	case 4 : return HitPrintSeg{ HP_CONST, '\n', 1 };
	case 5 : return HitPrintSeg{ HP_SID, 0, in.sid_len };
	// %-12s pads on the right; the blank in front of the score column
	case 6 : return HitPrintSeg{ HP_CONST, ' ', 1 + ( in.sid_len < HP_SID_WIDTH ? HP_SID_WIDTH - in.sid_len : 0 ) };
	case 7 : return HitPrintSeg{ HP_SCORE, 0, in.text_len };
	case 8 : return HitPrintSeg{ HP_NUM, 0, num_len };
	default : break;
	}
	const int	c = k - HP_FIRST_FIELD;
	if( c >= hitalign_n_cols( s ) )
		return HitPrintSeg{ HP_CONST, '\n', 1 };
	const int	x = hitstruct_word( s, hitalign_col_elem( s, c ) );
	return HitPrintSeg{ HP_FIELD, x, 1 + int64_t( hitalign_width( w[ x + 1 ] ) ) };
}

// the bytes of a checked record's two lines; 0 for a record that is not to be printed
RMW_FN int64_t hitprint_size( const int32_t *w, const HitWinShape &s, const HitPrintIn &in, bool accept )
{
	if( !accept )
		return 0;
	const int	num_len = hitprint_numbers( w, s, in.slen, nullptr, 0 ), n = hitprint_n_segs( s );
	int64_t	size = 0;
	for( int k = 0; k < n; k++ )
		size += hitprint_seg( w, s, in, num_len, k ).len;
	return size;
}

// Byte j (0 <= j < g.len) of segment g.  src: sid( j ), sdef( j ), score( j ), num( j ) -- the bytes of the name, the
// definition, the score column and hitprint_numbers' buffer -- and letter( p ), the letter at position p of the
// hit's strand.
template<class Src> RMW_FN uint8_t hitprint_seg_byte( const int32_t *w, const HitPrintSeg &g, int64_t j, const Src &src )
{
	switch( g.kind ){
	case HP_SID : return src.sid( j );
	case HP_SDEF : return src.sdef( j );
	case HP_SCORE : return src.score( j );
	case HP_NUM : return src.num( j );
	case HP_FIELD : return j == 0 ? ' ' : w[ g.arg + 1 ] <= 0 ? '.' : src.letter( w[ g.arg ] + int32_t( j - 1 ) );
	default : return uint8_t( g.arg );
	}
}

// byte b (0 <= b < hitprint_size) of the lines.  (The kernel lays the segments' offsets into LDS once per record and
// finds b's by bisection; it takes the same steps from there.)
template<class Src> RMW_FN uint8_t hitprint_byte( const int32_t *w, const HitWinShape &s, const HitPrintIn &in, int num_len, int64_t b, const Src &src )
{
	const int	n = hitprint_n_segs( s );
	for( int k = 0; k < n; k++ ){
		const HitPrintSeg	g = hitprint_seg( w, s, in, num_len, k );
		if( b < g.len )
			return hitprint_seg_byte( w, g, b, src );
		b -= g.len;
	}
	return 0;
}

// the last segment k of n whose first byte off[ k ] <= b: the segment byte b lies in, since no empty segment is the last
RMW_FN int hitprint_find_seg( const int64_t *off, int n, int64_t b )
{
	int	lo = 0, hi = n - 1;
	while( lo < hi ){
		const int	mid = ( lo + hi + 1 ) >> 1;
		if( off[ mid ] <= b )
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

// The record check: hitwin_span's, with its codes and *which, then HP_TEXT for a text_len outside [0, text_width].
RMW_FN int hitprint_check( const int32_t *w, const HitWinShape &s, int32_t n_seq, const int32_t *slen, int32_t text_len, int32_t text_width,
	int *which )
{
	int32_t	lo, hi;
	const int	r = hitwin_span( w, s, n_seq, slen, &lo, &hi, which );
	if( r != HW_OK )
		return r;
	return text_len < 0 || text_len > text_width ? int( HP_TEXT ) : int( HW_OK );
}

}	// namespace rma
