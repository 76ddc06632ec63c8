// rm_hitstruct.h -- the secondary structure of a hit record, base by base: which descriptor element a base of the
// record's window belongs to, and which bases it is matched with in the other strands of its helix.
//
// One rule for the host (tests/hostsim/hit_structures_check.cpp, the reasons rma_hit_structures() gives for a bad
// record) and the device (the fill kernel of rm_hitstruct_dev.hip).  The unit is the window of rm_hitwin.h: its span
// is hitwin_span's, its letters are hitwin_reader_letter's (or the code table's), strand 1 read from the 3' end and
// complemented.  For window index i of a record, position p = lo + i of the hit's strand:
//
//   elem     the index e of the element with off_e <= p < off_e + len_e; n_elems for the left context, n_elems + 1
//            for the right one, when the descriptor has them; -1 where nothing of positive length covers p.  The
//            elements of a record lie end to end; should two cover p (a record somebody made by hand), the LOWEST
//            index wins, the contexts last.
//   mate[3]  the window indices of the bases p is matched with in the other strands of its helix, the strands in
//            descriptor order (5' strand first) without p's own, padded with -1; all -1 for ss and the contexts.  The
//            other strands of an element are its rma_elem_t::mates[].  The geometry is the matcher's, with len the
//            common length of the strands:
//              duplex h5/h3      h5[ k ] pairs with h3[ len-1-k ]                   match_wchlx, find_motif.c:975
//              parallel p5/p3    p5[ k ] pairs with p3[ k ]                         match_phlx, find_motif.c:1114
//              triplex           t1[ k ], t2[ len-1-k ], t3[ k ]                    oracle/rm_oracle_scan.c:411-420,
//                                                                                   which restates find_motif.c:1183
//              4-plex            q1[ j ], q2[ len-1-j ], q3[ j ], q4[ len-1-j ]     oracle/rm_oracle_scan.c:447-457,
//                                                                                   find_motif.c:1234
//            that is: every strand has a direction, h3 / t2 / q2 / q4 run backwards, and the bases with the same
//            index counted along each strand's direction are matched.  A position the matcher counted as a mispair
//            still has its mates, as in a .ct file; n_mispairs is in the record.
//
// A record is checked before it is used: hitwin_span's checks (entry, strand, every extent, in 64 bits) and one
// more, HS_HELIX: the strands of one helix have the same length -- a mate is computed from len, and with equal
// lengths it lies inside its strand's extent, hence inside the window.
#pragma once
#include "rm_hitwin.h"

namespace rma {

// what the rule needs of one element of the program: its helix
struct HitStructElem {
	int8_t	n_strands;	// 0: ss (no mates), else the strands of its helix, 2-4
	int8_t	self;		// which of them this element is
	uint8_t	back;		// bit s: strand s runs backwards (h3, t2, q2, q4)
	int8_t	type;		// enum rma_type
	int16_t	strand[ 4 ];	// the helix's elements in descriptor order
};

// ... and of the program: 4 + 12 * RMA_MAX_ELEMS bytes, copied to the device as they are
struct HitStructTable {
	int32_t	n_elems;
	HitStructElem	e[ RMA_MAX_ELEMS ];
};

enum { HS_HELIX = HW_EXTENT + 1 };

inline HitStructTable hitstruct_table( const rma_program_t &p )
{
	HitStructTable	t;
	t.n_elems = p.n_elems;
	for( int e = 0; e < RMA_MAX_ELEMS; e++ ){
		HitStructElem	&x = t.e[ e ];
		x = HitStructElem{ 0, 0, 0, int8_t( RMA_T_SS ), { -1, -1, -1, -1 } };
		if( e >= p.n_elems )
			continue;
		const rma_elem_t	&el = p.elems[ e ];
		x.type = int8_t( el.type );
		if( el.type < RMA_T_H5 || el.type > RMA_T_Q4 || el.n_mates < 1 || el.n_mates > 3 )
			continue;
		// the helix in descriptor order: this element among its mates[]
		int	n = 0;
		bool	placed = false;
		for( int m = 0; m < el.n_mates; m++ ){
			if( !placed && e < el.mates[ m ] ){
				x.self = int8_t( n );
				x.strand[ n++ ] = int16_t( e );
				placed = true;
			}
			x.strand[ n++ ] = int16_t( el.mates[ m ] );
		}
		if( !placed ){
			x.self = int8_t( n );
			x.strand[ n++ ] = int16_t( e );
		}
		x.n_strands = int8_t( n );
		for( int s = 0; s < n; s++ ){
			const int	ty = p.elems[ x.strand[ s ] ].type;
			if( ty == RMA_T_H3 || ty == RMA_T_T2 || ty == RMA_T_Q2 || ty == RMA_T_Q4 )
				x.back = uint8_t( x.back | ( 1u << s ) );
		}
	}
	return t;
}

// the words of element e of a record (e = n_elems, n_elems + 1: the contexts): its offset is w[ k ], its length w[ k + 1 ]
RMW_FN int hitstruct_word( const HitWinShape &s, int e )
{
	return e < s.n_elems ? RMA_HIT_HDR + 4 * e : e == s.n_elems ? s.ctx_off : s.ctx_off + 2;
}

// whether the record has element e at all (a context the descriptor lacks is not there)
RMW_FN bool hitstruct_present( const HitWinShape &s, int e )
{
	return e < s.n_elems || ( e == s.n_elems && s.has_lctx ) || ( e == s.n_elems + 1 && s.has_rctx );
}

// an element at off of len bases covers position p
RMW_FN bool hitstruct_covers( int32_t off, int32_t len, int32_t p )
{
	return len > 0 && p >= off && int64_t( p ) < int64_t( off ) + len;
}

// hitwin_span and its checks, then HS_HELIX: *which the first strand (in descriptor order) whose length differs
// from that of its helix's 5' strand
RMW_FN int hitstruct_check( const int32_t *w, const HitStructTable &t, const HitWinShape &s, int32_t n_seq, const int32_t *slen,
	int32_t *lo, int32_t *hi, int *which )
{
	const int	r = hitwin_span( w, s, n_seq, slen, lo, hi, which );
	if( r != HW_OK )
		return r;
	for( int e = 0; e < s.n_elems; e++ ){
		const HitStructElem	&x = t.e[ e ];
		if( x.n_strands < 2 || x.self == 0 )
			continue;
		if( w[ RMA_HIT_HDR + 4 * e + 1 ] != w[ RMA_HIT_HDR + 4 * x.strand[ 0 ] + 1 ] ){
			*lo = 0;
			*hi = 0;
			*which = e;
			return HS_HELIX;
		}
	}
	return HW_OK;
}

// The mates of base k (0 <= k < len, counted from the element's 5' end) of an element x of len bases, in a window
// that starts at lo: soff[ s ] is the offset of strand s of x's helix (each of len bases: hitstruct_check).
RMW_FN void hitstruct_mates( const HitStructElem &x, int32_t k, int32_t len, const int32_t soff[ 4 ], int32_t lo, int32_t mate[ 3 ] )
{
	mate[ 0 ] = mate[ 1 ] = mate[ 2 ] = -1;
	if( x.n_strands < 2 )
		return;
	const int32_t	j = ( x.back >> x.self ) & 1 ? len - 1 - k : k;	// the index along the strand's direction
	int	n = 0;
	for( int s = 0; s < x.n_strands; s++ ){
		if( s == x.self )
			continue;
		mate[ n++ ] = soff[ s ] + ( ( x.back >> s ) & 1 ? len - 1 - j : j ) - lo;
	}
}

// The rule for one base of a checked record, from the record's words: window index i of the window that starts
// at lo.  (The kernel holds the record's offsets and lengths in registers and walks them in the same order.)
RMW_FN void hitstruct_base( const int32_t *w, const HitStructTable &t, const HitWinShape &s, int32_t lo, int64_t i, int *elem, int32_t mate[ 3 ] )
{
	const int32_t	p = int32_t( lo + i );
	int	e = -1;
	for( int c = s.n_elems + 1; c >= 0; c-- ){		// (downwards: the lowest index that covers p stays)
		const int	k = hitstruct_word( s, c );
		if( hitstruct_present( s, c ) && hitstruct_covers( w[ k ], w[ k + 1 ], p ) )
			e = c;
	}
	*elem = e;
	mate[ 0 ] = mate[ 1 ] = mate[ 2 ] = -1;
	if( e < 0 || e >= s.n_elems )
		return;
	const HitStructElem	&x = t.e[ e ];
	int32_t	soff[ 4 ] = { 0, 0, 0, 0 };
	for( int q = 0; q < x.n_strands; q++ )
		soff[ q ] = w[ RMA_HIT_HDR + 4 * x.strand[ q ] ];
	hitstruct_mates( x, p - w[ RMA_HIT_HDR + 4 * e ], w[ RMA_HIT_HDR + 4 * e + 1 ], soff, lo, mate );
}

}	// namespace rma
