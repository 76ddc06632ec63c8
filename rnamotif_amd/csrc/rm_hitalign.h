// rm_hitalign.h -- a set of hit records as an alignment: the byte matrix whose rows, cut into lines of 70, are the
// sequence lines `rmfmt -a` writes for the printed form of the same records (align(), rmfmt.c:531-554).
//
// One rule for the host (tests/hostsim/hit_align_check.cpp, the widths rma_hit_alignment() holds a caller to) and
// the device (the widths and fill kernels of rm_hitalign_dev.hip).
//
//   columns   stand in the order print_match() prints fields (find_motif.c:1869-1896): the left context when the
//             descriptor has one, elements 0 .. n_elems-1, the right context when it has one -- at most
//             RMA_MAX_ELEMS + 2.  Column c's element is hitalign_col_elem(), numbered as rm_hitstruct.h numbers
//             them (n_elems: the left context, n_elems + 1: the right one).
//   width     of a field: the length of its printed form, len for len > 0 and 1 for an empty element, which is
//             printed as "." (hitalign_width).  Of a column: the maximum over the records given, so never below 1
//             when there is a record.
//   direction a column is right-aligned exactly when its element's type is h3, t2, q2 or q4: getfmt(),
//             rmfmt.c:418-425, which reads the first two characters of the "#RM descr" name.  The contexts and
//             everything else are left-aligned.  (-a does not abbreviate long fields: fcmprs does not apply.)
//   row       W = the sum of the widths + n_cols - 1 bytes: the fields in column order, each padded to its column's
//             width with the gap byte on its free side, one separator byte between neighbouring columns.  The
//             defaults are '-', '|' and '.', the tool's own.
//   pos       for a letter byte the position on the hit's strand it came from, in the coordinate hit_structures'
//             lo uses: the element's offset + the letter's index in the field; -1 for gap, separator and "." bytes.
//             The letter is hitwin's: the reader's letter or the table's, on strand 1 read from the 3' end of the
//             entry (hitwin_src) and complemented.
//
// A record is checked by hitwin_span's checks before anything of it is used; equal strand lengths within a helix
// are NOT required, because rmfmt does not require them.
#pragma once
#include "rm_hitwin.h"
#include "rm_hitstruct.h"

namespace rma {

enum { HA_MAX_COLS = RMA_MAX_ELEMS + 2 };
enum { HA_SEP = 0, HA_GAP, HA_DOT, HA_LETTER };		// what a byte of a row is
enum { HA_FILL_GAP = 0, HA_FILL_SEP, HA_FILL_EMPTY };	// the bytes of fill[ 3 ]

RMW_FN int hitalign_n_cols( const HitWinShape &s )
{
	return s.n_elems + ( s.has_lctx ? 1 : 0 ) + ( s.has_rctx ? 1 : 0 );
}

// the element of column c (0 <= c < hitalign_n_cols), numbered as hitstruct_word() takes it
RMW_FN int hitalign_col_elem( const HitWinShape &s, int c )
{
	const int	e = c - ( s.has_lctx ? 1 : 0 );
	return e < 0 ? s.n_elems : e >= s.n_elems ? s.n_elems + 1 : e;
}

// the width of a field of len bases as it is printed
RMW_FN int32_t hitalign_width( int32_t len )
{
	return len > 0 ? len : 1;
}

// getfmt(): the types whose columns are right-aligned
RMW_FN bool hitalign_type_right( int type )
{
	return type == RMA_T_H3 || type == RMA_T_T2 || type == RMA_T_Q2 || type == RMA_T_Q4;
}

// The columns of a row: column c is bytes [ off[ c ], off[ c ] + width[ c ] ), the separator behind it (c < n_cols - 1)
// byte off[ c ] + width[ c ]; row_bytes = W.  Handed to the fill kernel as it is.
struct HitAlignLayout {
	int64_t	off[ HA_MAX_COLS ];
	int64_t	row_bytes;
	int32_t	width[ HA_MAX_COLS ];
	int32_t	n_cols;
	uint8_t	right[ HA_MAX_COLS ];
	uint8_t	fill[ 3 ];
	uint8_t	pad_[ 3 ];
};

// the directions of a program's columns
inline void hitalign_directions( const rma_program_t &p, uint8_t right[ HA_MAX_COLS ] )
{
	const HitWinShape	s = hitwin_shape( p );
	const int	n = hitalign_n_cols( s );
	for( int c = 0; c < HA_MAX_COLS; c++ ){
		const int	e = c < n ? hitalign_col_elem( s, c ) : s.n_elems;
		right[ c ] = e < s.n_elems && hitalign_type_right( p.elems[ e ].type ) ? 1 : 0;
	}
}

// the layout of rows whose columns have these widths (each >= 0); fill: gap, separator, empty
inline HitAlignLayout hitalign_layout( const rma_program_t &p, const int32_t *widths, const uint8_t fill[ 3 ] )
{
	HitAlignLayout	l;
	const int	n = hitalign_n_cols( hitwin_shape( p ) );
	l.n_cols = n;
	hitalign_directions( p, l.right );
	int64_t	at = 0;
	for( int c = 0; c < HA_MAX_COLS; c++ ){
		l.width[ c ] = c < n ? widths[ c ] : 0;
		l.off[ c ] = at;
		if( c < n )
			at += int64_t( l.width[ c ] ) + ( c < n - 1 ? 1 : 0 );
	}
	l.row_bytes = at;
	for( int k = 0; k < 3; k++ ){
		l.fill[ k ] = fill[ k ];
		l.pad_[ k ] = 0;
	}
	return l;
}

// the column byte b (0 <= b < W) of a row lies in, its separator included: the last c with off[ c ] <= b
RMW_FN int hitalign_find_col( const int64_t *off, int n_cols, int64_t b )
{
	int	lo = 0, hi = n_cols - 1;
	while( lo < hi ){
		const int	mid = ( lo + hi + 1 ) >> 1;
		if( off[ mid ] <= b )
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

// Byte j (0 <= j <= width) of a column of this width and direction that holds a field of len bases: what it is, and
// for HA_LETTER the letter's index *k in the field.  j == width is the separator behind the column.
RMW_FN int hitalign_place( int32_t width, int right, int32_t len, int64_t j, int32_t *k )
{
	*k = 0;
	if( j >= width )
		return HA_SEP;
	const int32_t	f = hitalign_width( len );
	const int64_t	first = right ? int64_t( width ) - f : 0;
	if( j < first || j >= first + f )
		return HA_GAP;
	if( len <= 0 )
		return HA_DOT;
	*k = int32_t( j - first );
	return HA_LETTER;
}

// The rule for one byte of a checked record's row, from the record's words: byte b of a row of layout l.  Returns
// what it is; for HA_LETTER *pos is the letter's position on the hit's strand (else -1).  (The kernel holds the
// record's offsets and lengths in registers and takes the same steps.)
RMW_FN int hitalign_byte( const int32_t *w, const HitWinShape &s, const HitAlignLayout &l, int64_t b, int32_t *pos )
{
	const int	c = hitalign_find_col( l.off, l.n_cols, b );
	const int	x = hitstruct_word( s, hitalign_col_elem( s, c ) );
	int32_t	k;
	const int	kind = hitalign_place( l.width[ c ], l.right[ c ], w[ x + 1 ], b - l.off[ c ], &k );
	*pos = kind == HA_LETTER ? w[ x ] + k : -1;
	return kind;
}

// the byte a row holds where hitalign_byte() says something other than HA_LETTER
RMW_FN uint8_t hitalign_fill_byte( const uint8_t fill[ 3 ], int kind )
{
	return kind == HA_SEP ? fill[ HA_FILL_SEP ] : kind == HA_GAP ? fill[ HA_FILL_GAP ] : fill[ HA_FILL_EMPTY ];
}

}	// namespace rma
