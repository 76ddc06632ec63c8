// rm_prune.h -- which hit records are only "unzipped" versions of another record: the rule of the rmprune tool
// (tools/rmprune.cpp, which cites rmprune.c line by line), restated over records instead of printed text.
//
// One rule for the host (prune_mask below: tests/hostsim/prune_check.cpp) and the device (the kernels of
// rm_prune_dev.hip, rma_prune_hits).  The answer is a keep flag per record, the one decision the tool makes on the
// printed form of the same records in the same order; every quirk of the tool is kept, for the test is equality.
//
//   printed coordinates   start = comp ? slen[ seq ] - off_0 : off_0 + 1 (off_0: element 0's offset), len the sum of
//     (HitPrinter::print)  the elements' lengths without the contexts, stop = comp ? start - len + 1 : start + len - 1
//   element spans         locate() does not read offsets: it walks the printed fields -- the left context if the
//     (locate)             descriptor has one, the elements, the right context -- and gives field f
//                          start +- done .. that +- (flen - 1), "-" on strand 1, done the sum of flen over the fields
//                          before it, flen the field's length and 1 WHERE THE LENGTH IS 0 (the printed ".").  So a
//                          left context shifts every element and an empty element those behind it.
//   groups of strands     read_descr(): tagged strands by tag, untagged h5/p5 with the next untagged element that is
//     (PruneTable)         not ss, by a stack.  For a descriptor the compiler accepts that is an element's mates[]
//                          (tests/test_prune_cpu.py holds the table to read_descr() on every descriptor of the corpus).
//   relation of two hits  relation() / helix_relation(), rmprune.cpp:150-209: a duplex by its h5 and group[ 1 ]; p5,
//                          t1, q1 by equality of all strands' spans; every other element says SAME; contexts are
//                          skipped.  DOWN against LEFT is DIFF; comp is that of the later hit.  Only the judged
//                          elements are walked here: SAME from the others can only turn "nothing yet" into SAME, and
//                          rezip treats the two alike.
//   runs and blocks       consecutive records whose entries have the same name group are a run, a run is cut into
//                          blocks of PRUNE_BLOCK records; inside a block everything from the first record with
//                          comp != 0 on is taken as strand 1, whatever its comp; a new group starts where a record
//                          leaves the leader's span (start < g.start || stop > g.stop; from first_comp on start >
//                          g.start || stop < g.stop); rezip() per group: b from last to second, if kept, b1 from b - 1
//                          down, if kept: DOWN drops b1, LEFT drops b and ends b's pass.
//
// A record is checked before it is used: hitwin_span's checks (entry, strand, every extent, in 64 bits).
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>
#include "rm_hitstruct.h"

namespace rma {

enum { PRUNE_BLOCK = 1000 };					// BLOCK_SIZE, rmprune.c
enum { PR_SAME = 0, PR_LEFT, PR_DOWN, PR_DIFF };		// rmprune.c:86-90, "none yet" counted as SAME
enum { PRUNE_MAX_FIELDS = RMA_MAX_ELEMS + 2 };

// one judged element: a duplex (its h5's slot and group[ 1 ]'s) or a p5 / t1 / q1 (all its strands' slots)
struct PruneJudged {
	int8_t	duplex, n;
	int16_t	slot[ 4 ];		// places in a record's key row, see prune_keys
	int16_t	pad;
};

// What the rule needs of the program, copied to the device as it is.  A printed field is a context or an element;
// a helix strand among them has a slot, its place in the key row of a record.
struct PruneTable {
	int32_t	n_fields, n_slots, n_judged, has_lctx;
	PruneJudged	judged[ RMA_MAX_ELEMS ];		// (behind the four words: the kernel copies them word by word)
	int8_t	kind[ PRUNE_MAX_FIELDS ];		// the tool's K_*: enum rma_type's numbers, 0 for a context
	int16_t	slot[ PRUNE_MAX_FIELDS ];		// -1: not a helix strand
	int16_t	group[ PRUNE_MAX_FIELDS ][ 4 ];		// read_descr()'s group[]: printed-field indices, -1 padding
};
static_assert( sizeof( PruneJudged ) == 12 && offsetof( PruneTable, judged ) == 16, "the judged elements lie on a word boundary" );

inline PruneTable prune_table( const rma_program_t &p )
{
	PruneTable	t;
	memset( &t, 0, sizeof( t ) );
	const HitStructTable	hs = hitstruct_table( p );
	const int	shift = p.has_lctx ? 1 : 0;
	t.has_lctx = shift;
	t.n_fields = p.n_elems + shift + ( p.has_rctx ? 1 : 0 );
	for( int f = 0; f < PRUNE_MAX_FIELDS; f++ ){
		t.kind[ f ] = int8_t( RMA_T_CTX );
		t.slot[ f ] = -1;
		for( int i = 0; i < 4; i++ )
			t.group[ f ][ i ] = -1;
	}
	for( int e = 0; e < p.n_elems; e++ ){
		const int	f = e + shift, ty = p.elems[ e ].type;
		t.kind[ f ] = int8_t( ty );
		if( ty >= RMA_T_H5 && ty <= RMA_T_Q4 ){
			t.slot[ f ] = int16_t( t.n_slots++ );
			for( int i = 0; i < hs.e[ e ].n_strands; i++ )
				t.group[ f ][ i ] = int16_t( hs.e[ e ].strand[ i ] + shift );
		}
	}
	for( int e = 0; e < p.n_elems; e++ ){
		const int	f = e + shift, ty = t.kind[ f ];
		PruneJudged	q{ 0, 0, { -1, -1, -1, -1 }, 0 };
		if( ty == RMA_T_H5 && t.group[ f ][ 1 ] >= 0 ){
			q.duplex = 1;
			q.n = 2;
			q.slot[ 0 ] = t.slot[ f ];
			q.slot[ 1 ] = t.slot[ t.group[ f ][ 1 ] ];
		}else if( ty == RMA_T_P5 || ty == RMA_T_T1 || ty == RMA_T_Q1 ){
			for( int i = 0; i < 4 && t.group[ f ][ i ] >= 0; i++ )
				q.slot[ q.n++ ] = t.slot[ t.group[ f ][ i ] ];
		}else
			continue;
		t.judged[ t.n_judged++ ] = q;
	}
	return t;
}

// the words of printed field f of a record: its length is w[ k + 1 ]
RMW_FN int prune_field_word( const PruneTable &t, const HitWinShape &s, int f )
{
	const int	e = f - t.has_lctx;
	return e < 0 ? s.ctx_off : e < s.n_elems ? RMA_HIT_HDR + 4 * e : s.ctx_off + 2;
}

// 32-bit sums as the tool's ints, without the undefined overflow
RMW_FN int32_t prune_add( int32_t a, int32_t b )
{
	return int32_t( uint32_t( a ) + uint32_t( b ) );
}

// The keys of a checked record w of an entry of slen bases: css[ 3 ] = comp, start, stop as printed, and the key
// row, row[ 2 * slot ] / row[ 2 * slot + 1 ] = the start / stop locate() gives the helix strand with that slot.
RMW_FN void prune_keys( const int32_t *w, const PruneTable &t, const HitWinShape &s, int32_t slen, int32_t css[ 3 ], int32_t *row )
{
	const int	comp = w[ 1 ];
	int32_t	len = 0;
	for( int e = 0; e < s.n_elems; e++ )
		len = prune_add( len, w[ RMA_HIT_HDR + 4 * e + 1 ] );
	const int32_t	start = comp ? prune_add( slen, -w[ RMA_HIT_HDR ] ) : prune_add( w[ RMA_HIT_HDR ], 1 );
	css[ 0 ] = comp;
	css[ 1 ] = start;
	css[ 2 ] = comp ? prune_add( prune_add( start, -len ), 1 ) : prune_add( prune_add( start, len ), -1 );
	int32_t	done = 0;
	for( int f = 0; f < t.n_fields; f++ ){
		const int32_t	l = w[ prune_field_word( t, s, f ) + 1 ], flen = l == 0 ? 1 : l;
		const int	sl = t.slot[ f ];
		if( sl >= 0 ){
			const int32_t	a = comp ? prune_add( start, -done ) : prune_add( start, done );
			row[ 2 * sl ] = a;
			row[ 2 * sl + 1 ] = comp ? prune_add( prune_add( a, -flen ), 1 ) : prune_add( prune_add( a, flen ), -1 );
		}
		done = prune_add( done, flen );
	}
}

// helix_relation(), rmprune.cpp:150: a and b the key rows' ( start, stop ) of the 5' and the 3' strand
RMW_FN int prune_helix_relation( int comp, const int32_t *a5, const int32_t *a3, const int32_t *b5, const int32_t *b3 )
{
	int64_t	lod, rod, lid, rid;	// left/right, outer/inner differences
	if( !comp ){
		lod = int64_t( b5[ 0 ] ) - a5[ 0 ];
		rod = int64_t( a3[ 1 ] ) - b3[ 1 ];
		lid = int64_t( a5[ 1 ] ) - b5[ 1 ];
		rid = int64_t( b3[ 0 ] ) - a3[ 0 ];
	}else{
		lod = int64_t( a5[ 0 ] ) - b5[ 0 ];
		rod = int64_t( b3[ 1 ] ) - a3[ 1 ];
		lid = int64_t( b5[ 1 ] ) - a5[ 1 ];
		rid = int64_t( a3[ 0 ] ) - b3[ 0 ];
	}
	if( lod != rod || lid != rid )
		return PR_DIFF;
	if( lod > 0 )
		return lid < 0 ? PR_DIFF : PR_DOWN;
	if( lod == 0 )
		return lid < 0 ? PR_LEFT : lid == 0 ? PR_SAME : PR_DOWN;
	return lid < 0 ? PR_DIFF : PR_LEFT;
}

// relation(), rmprune.cpp:173, of hit a (the later one, on strand comp) and hit b by their key rows
RMW_FN int prune_relation( const PruneJudged *judged, int n_judged, int comp, const int32_t *a, const int32_t *b )
{
	int	rel = PR_SAME;
	for( int j = 0; j < n_judged; j++ ){
		const PruneJudged	&q = judged[ j ];
		int	r1 = PR_SAME;
		if( q.duplex )
			r1 = prune_helix_relation( comp, a + 2 * q.slot[ 0 ], a + 2 * q.slot[ 1 ], b + 2 * q.slot[ 0 ], b + 2 * q.slot[ 1 ] );
		else
			for( int i = 0; i < q.n; i++ ){
				const int	k = 2 * q.slot[ i ];
				if( a[ k ] != b[ k ] || a[ k + 1 ] != b[ k + 1 ] ){
					r1 = PR_DIFF;
					break;
				}
			}
		if( r1 == PR_DIFF )
			return PR_DIFF;
		if( rel == PR_SAME )
			rel = r1;
		else if( ( rel == PR_DOWN && r1 == PR_LEFT ) || ( rel == PR_LEFT && r1 == PR_DOWN ) )
			return PR_DIFF;
	}
	return rel;
}

// a record of ( start, stop ) leaves the span ( gs, ge ) of its group's leader; strand1: from first_comp on
RMW_FN bool prune_leaves( bool strand1, int32_t start, int32_t stop, int32_t gs, int32_t ge )
{
	return strand1 ? start > gs || stop < ge : start < gs || stop > ge;
}

#if !defined( __HIP_DEVICE_COMPILE__ )
// what the host's pass counts
struct PruneCounts {
	int64_t	down = 0, left = 0, blocks = 0, groups = 0;
};

// The whole rule on the host, record by record as the tool goes: keep[ n ] for the n records at recs (stride words
// each) of entries of slen[ n_seq ] bases, group_of_entry[ n_seq ] or null (an entry's own index).  Returns -1, or
// the index of the first record hitwin_span refuses (nothing is judged then).
inline int64_t prune_mask( const int32_t *recs, int64_t n, int stride, const rma_program_t &prog, int32_t n_seq, const int32_t *slen,
	const int32_t *group_of_entry, uint8_t *keep, PruneCounts *counts )
{
	const PruneTable	t = prune_table( prog );
	const HitWinShape	shape = hitwin_shape( prog );
	const size_t	row = size_t( 2 * ( t.n_slots > 0 ? t.n_slots : 1 ) );
	std::vector<int32_t>	css( size_t( n ) * 3 ), rows( size_t( n ) * row );
	for( int64_t h = 0; h < n; h++ ){
		int32_t	lo, hi;
		int	which;
		const int32_t	*w = recs + h * stride;
		if( hitwin_span( w, shape, n_seq, slen, &lo, &hi, &which ) != HW_OK )
			return h;
		prune_keys( w, t, shape, slen[ w[ 0 ] ], &css[ size_t( h ) * 3 ], &rows[ size_t( h ) * row ] );
		keep[ h ] = 1;
	}
	PruneCounts	c;
	auto gid = [&]( int64_t h ){ const int32_t e = recs[ h * stride ]; return group_of_entry != nullptr ? group_of_entry[ e ] : e; };
	auto rezip = [&]( int64_t lb, int64_t end ){
		c.groups += end > lb;
		for( int64_t b = end - 1; b > lb; b-- ){
			if( !keep[ b ] )
				continue;
			for( int64_t b1 = b - 1; b1 >= lb; b1-- ){
				if( !keep[ b1 ] )
					continue;
				const int	r = prune_relation( t.judged, t.n_judged, css[ size_t( b ) * 3 ], &rows[ size_t( b ) * row ], &rows[ size_t( b1 ) * row ] );
				if( r == PR_DOWN ){
					keep[ b1 ] = 0;
					c.down++;
				}else if( r == PR_LEFT ){
					keep[ b ] = 0;
					c.left++;
					break;
				}
			}
		}
	};
	for( int64_t s = 0; s < n; ){
		int64_t	e = s + 1;
		while( e < n && e - s < PRUNE_BLOCK && gid( e ) == gid( s ) )
			e++;
		c.blocks++;
		int64_t	fc = s;
		while( fc < e && !css[ size_t( fc ) * 3 ] )
			fc++;
		for( int sec = 0; sec < 2; sec++ ){
			const int64_t	from = sec ? fc : s, to = sec ? e : fc;
			for( int64_t lb = from; lb < to; ){
				const int32_t	gs = css[ size_t( lb ) * 3 + 1 ], ge = css[ size_t( lb ) * 3 + 2 ];
				int64_t	b = lb + 1;
				while( b < to && !prune_leaves( sec != 0, css[ size_t( b ) * 3 + 1 ], css[ size_t( b ) * 3 + 2 ], gs, ge ) )
					b++;
				rezip( lb, b );
				lb = b;
			}
		}
		s = e;
	}
	if( counts != nullptr )
		*counts = c;
	return -1;
}
#endif

}	// namespace rma
