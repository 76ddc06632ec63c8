// rm_hitlist.h -- the listing of hit records: what rmfmt (rmfmt.c:122-353, -a off) makes of rnamotif's output for them --
// the hits in sort(1)'s order under rmfmt's keys, every field padded to its widest instance -- as bytes.
//
// One rule for the host (tests/hostsim/hit_list_check.cpp, the reasons rma_hit_list() gives for a refusal) and the
// device (the measure kernel, the comparator of the sort and the fill kernel of rm_hitlist_dev.hip).  For record w of
// a program, of an entry of slen bases named sid, whose score column is the text_len bytes rma_score_hits_text()
// delivers:
//
//   name          the sid, trimmed as rmfmt.c:188-217 does: whole; locus (-l): the text after the last '|', else the
//                 text between the last two, else the text in front of the only one; accession (-la): the text between
//                 the last two '|', a name with fewer than two whole -- a span (start, length) of the sid
//   score fields  the tokens of the score column, split on blank and tab; K of them, joined by single blanks:
//                 the sum of their lengths + K - 1 bytes wide
//   comp, offset, len   rm_hitprint.h's, as plain %d
//   fields        one per column of rm_hitalign.h: the element's letters, "." for an empty one; more than 20 letters
//                 become the first 3, "...(N)..." and the last 3 (fcmprs), and that form is the field everywhere below
//   temp line     what rmfmt writes to its raw temp file: name, score fields, the three numbers, the fields, joined by
//                 single blanks, "\n"; the sum of their lengths over the printed records is the size -smax is held to
//   mode          0 (input order) where the temp bytes exceed smax; else 1 where K is 1 and every printed record's
//                 token is a number by is_a_number (rmfmt.c:431-461); else 2
//   order         rmlist_less: sort(1) in the C locale with "-k 2rn,2 -k 1,1 -k 3n,3 -k 4n,4 -k 5n,5" (mode 1) or
//                 "-k 1,1" and the three numbers behind the score fields (mode 2), then sort's last resort, the whole
//                 temp line by bytes, then the record's index
//   line          the name left-justified in the widest name's width; a blank; the score block (K 1: right-justified,
//                 else padded on the right); for comp, offset, len and every field a blank and the text right- or
//                 left-justified in its column's width (numbers right; fields right for h3, t2, q2, q4); "\n" -- every
//                 line of a listing has the same length
//
// A line's parts are its segments: HL_NAME, HL_SCORE, HL_COMP, HL_OFFSET, HL_LEN and one per field, at most 107.
// What the reference's result is not a function of its input for is refused, not restated: records whose K differ (the
// sort command is written with the last line's n_sfields) and an empty score column (a stale sfields[ 0 ]) --
// bin/rmfmt resolves both in its own way.  A newline inside a score column, a line of more than MAXFIELDS fields and a
// hit line of LINE_SIZE bytes or more are refused as well.
#pragma once
#include <cstdio>
#include "rm_hitprint.h"

namespace rma {

enum { HL_WHOLE = 0, HL_LOCUS, HL_ACC };					// rmfmt, rmfmt -l, rmfmt -la
enum { HL_NAME = 0, HL_SCORE, HL_COMP, HL_OFFSET, HL_LEN, HL_FIRST_FIELD, HL_MAX_SEGS = HL_FIRST_FIELD + HA_MAX_COLS };
enum { HL_MAXW = 20, HL_MAXFIELDS = 200, HL_LINE_SIZE = 50000 };	// rmfmt.c's MAXW, MAXFIELDS, LINE_SIZE
// what refuses a record, behind hitprint_check's codes
enum { HL_EMPTY = HP_TEXT + 1, HL_NEWLINE, HL_FIELDS, HL_LINE };
enum { HL_F_NUMBER = 1 };
constexpr int64_t	HL_SMAX = 30000000;

// what the measure pass keeps of a printed record (k < 0: not printed)
struct HitListRec {
	int32_t	name_at, name_len;	// the trimmed name inside the sid
	int32_t	k;			// score fields
	int32_t	tok_at, score_w;	// the first token's first byte in the column; the joined tokens' bytes
	int32_t	num[ 3 ];		// comp, offset, len
	int32_t	temp_len;		// the temp line's bytes
	int32_t	flags;			// HL_F_NUMBER: K is 1 and the token is a number
};

// the columns of a listing; handed to the fill kernel as it is
struct HitListLayout {
	int32_t	off[ HL_MAX_SEGS ];	// a segment's first byte (behind its blank)
	int32_t	width[ HL_MAX_SEGS ];
	uint8_t	right[ HL_MAX_SEGS ];
	int32_t	n_segs, k, line_len;
};

RMW_FN int rmlist_n_segs( const HitWinShape &s )
{
	return HL_FIRST_FIELD + hitalign_n_cols( s );
}

// the trimmed name of a sid of n bytes: its length, *at its first byte
RMW_FN int32_t rmlist_name( const uint8_t *sid, int32_t n, int mode, int32_t *at )
{
	*at = 0;
	if( mode == HL_WHOLE )
		return n;
	int32_t	last = -1, prev = -1;
	for( int32_t i = 0; i < n; i++ )
		if( sid[ i ] == '|' ){
			prev = last;
			last = i;
		}
	if( last < 0 )
		return n;
	if( mode == HL_LOCUS && last + 1 < n ){
		*at = last + 1;
		return n - last - 1;
	}
	if( prev >= 0 ){
		*at = prev + 1;
		return last - prev - 1;
	}
	return mode == HL_LOCUS ? last : n;
}

RMW_FN bool rmlist_blank( uint8_t c )
{
	return c == ' ' || c == '\t';
}

// the next token of a score column of n bytes at or behind *pos: its length (0: none), *at its first byte
RMW_FN int32_t rmlist_token( const uint8_t *col, int32_t n, int32_t *pos, int32_t *at )
{
	int32_t	i = *pos;
	while( i < n && rmlist_blank( col[ i ] ) )
		i++;
	*at = i;
	while( i < n && !rmlist_blank( col[ i ] ) )
		i++;
	*pos = i;
	return i - *at;
}

RMW_FN bool rmlist_digit( uint8_t c )
{
	return c >= '0' && c <= '9';
}

// is_a_number( rmfmt.c:431-461 ) of a token of n bytes
RMW_FN bool rmlist_is_number( const uint8_t *p, int32_t n )
{
	int32_t	i = 0, mant = 0, expo = 0;
	bool	efmt = false;
	if( i < n && p[ i ] == '-' )
		i++;
	for( ; i < n && rmlist_digit( p[ i ] ); i++ )
		mant++;
	if( i < n && p[ i ] == '.' )
		i++;
	for( ; i < n && rmlist_digit( p[ i ] ); i++ )
		mant++;
	if( i < n && ( p[ i ] == 'e' || p[ i ] == 'E' ) ){
		efmt = true;
		i++;
		if( i < n && p[ i ] == '-' )
			i++;
		for( ; i < n && rmlist_digit( p[ i ] ); i++ )
			expo++;
	}
	return mant > 0 && !( efmt && expo == 0 ) && i == n;
}

// What sort -n reads of a token: an optional '-', digits, an optional '.' and digits; nothing behind that counts.
// The integer part without its leading zeros, the fraction without its trailing ones; neither: the number is 0.
struct HitListNum {
	int32_t	int_at, int_len, frac_at, frac_len;
	bool	neg;
};

RMW_FN HitListNum rmlist_sort_number( const uint8_t *p, int32_t n )
{
	HitListNum	v{ 0, 0, 0, 0, false };
	int32_t	i = 0;
	if( i < n && p[ i ] == '-' ){
		v.neg = true;
		i++;
	}
	while( i < n && p[ i ] == '0' )
		i++;
	v.int_at = i;
	while( i < n && rmlist_digit( p[ i ] ) )
		i++;
	v.int_len = i - v.int_at;
	if( i < n && p[ i ] == '.' ){
		v.frac_at = ++i;
		int32_t	end = i;
		for( ; i < n && rmlist_digit( p[ i ] ); i++ )
			if( p[ i ] != '0' )
				end = i + 1;
		v.frac_len = end - v.frac_at;
	}
	if( v.int_len == 0 && v.frac_len == 0 )
		v.neg = false;		// -0.000 is 0.000
	return v;
}

// -1, 0, 1: the numbers of two tokens as exact decimals
RMW_FN int rmlist_number_cmp( const uint8_t *pa, int32_t na, const uint8_t *pb, int32_t nb )
{
	const HitListNum	a = rmlist_sort_number( pa, na ), b = rmlist_sort_number( pb, nb );
	if( a.neg != b.neg )
		return a.neg ? -1 : 1;
	int	c = 0;
	if( a.int_len != b.int_len )
		c = a.int_len < b.int_len ? -1 : 1;
	for( int32_t i = 0; c == 0 && i < a.int_len; i++ )
		if( pa[ a.int_at + i ] != pb[ b.int_at + i ] )
			c = pa[ a.int_at + i ] < pb[ b.int_at + i ] ? -1 : 1;
	const int32_t	m = a.frac_len < b.frac_len ? a.frac_len : b.frac_len;
	for( int32_t i = 0; c == 0 && i < m; i++ )
		if( pa[ a.frac_at + i ] != pb[ b.frac_at + i ] )
			c = pa[ a.frac_at + i ] < pb[ b.frac_at + i ] ? -1 : 1;
	// (no trailing zeros: the longer fraction is the larger one)
	if( c == 0 && a.frac_len != b.frac_len )
		c = a.frac_len < b.frac_len ? -1 : 1;
	return a.neg ? -c : c;
}

RMW_FN int32_t rmlist_digits( int32_t v )
{
	uint32_t	u = v < 0 ? 0u - uint32_t( v ) : uint32_t( v );
	int32_t	n = v < 0 ? 2 : 1;
	for( ; u >= 10; u /= 10 )
		n++;
	return n;
}

// byte j (0 <= j < rmlist_digits( v )) of %d of v
RMW_FN uint8_t rmlist_digit_byte( int32_t v, int32_t j )
{
	if( v < 0 && j == 0 )
		return '-';
	uint32_t	u = v < 0 ? 0u - uint32_t( v ) : uint32_t( v );
	for( int32_t k = rmlist_digits( v ) - 1 - j; k > 0; k-- )
		u /= 10;
	return uint8_t( '0' + u % 10 );
}

// the width of the field of an element of len letters: ".", the letters, or fcmprs' form
RMW_FN int32_t rmlist_field_width( int32_t len )
{
	return len <= 0 ? 1 : len <= HL_MAXW ? len : 3 + 4 + rmlist_digits( len ) + 4 + 3;
}

// byte j of the field of the element at off of len letters; let.letter( p ): the letter at position p of the strand
template<class Let> RMW_FN uint8_t rmlist_field_byte( int32_t off, int32_t len, int32_t j, const Let &let )
{
	if( len <= 0 )
		return '.';
	if( len <= HL_MAXW )
		return let.letter( off + j );
	const int32_t	nd = rmlist_digits( len );
	if( j < 3 )
		return let.letter( off + j );
	if( j < 7 )
		return j == 6 ? '(' : '.';
	if( j < 7 + nd )
		return rmlist_digit_byte( len, j - 7 );
	if( j < 11 + nd )
		return j == 7 + nd ? ')' : '.';
	return let.letter( off + len - 3 + ( j - 11 - nd ) );
}

// comp, offset or len of a measured record, by its segment (no indexed access: the record stays in registers)
RMW_FN int32_t rmlist_num( const HitListRec &r, int g )
{
	return g == HL_COMP ? r.num[ 0 ] : g == HL_OFFSET ? r.num[ 1 ] : r.num[ 2 ];
}

// the record word of field segment g (g >= HL_FIRST_FIELD): its element's offset, the length behind it
RMW_FN int rmlist_field_word( const HitWinShape &s, int g )
{
	return hitstruct_word( s, hitalign_col_elem( s, g - HL_FIRST_FIELD ) );
}

// A record hitprint_check has passed, measured: HW_OK and *r, or what refuses it.  in: its entry's name lengths and
// bases and its text_len (rm_hitprint.h); sid, col: the bytes of its entry's name and of its score column.
RMW_FN int rmlist_measure( const int32_t *w, const HitWinShape &s, const HitPrintIn &in, const uint8_t *sid, const uint8_t *col, int mode,
	HitListRec *r )
{
	r->name_len = rmlist_name( sid, int32_t( in.sid_len ), mode, &r->name_at );
	r->k = 0;
	r->tok_at = 0;
	r->score_w = 0;
	for( int32_t i = 0; i < in.text_len; i++ )
		if( col[ i ] == '\n' )
			return HL_NEWLINE;
	int32_t	pos = 0, at = 0, first = 0;
	for( int32_t n; ( n = rmlist_token( col, in.text_len, &pos, &at ) ) > 0; r->k++ ){
		if( r->k == 0 ){
			r->tok_at = at;
			first = n;
		}
		r->score_w += n + ( r->k > 0 ? 1 : 0 );
	}
	if( r->k == 0 )
		return HL_EMPTY;
	const int	nc = hitalign_n_cols( s );
	if( int64_t( 1 ) + r->k + 3 + nc > HL_MAXFIELDS )
		return HL_FIELDS;
	// the hit line as rnamotif prints it: the record's two lines without the definition line
	if( hitprint_size( w, s, in, true ) - ( 3 + in.sid_len + in.sdef_len ) >= HL_LINE_SIZE )
		return HL_LINE;
	r->flags = r->k == 1 && rmlist_is_number( col + r->tok_at, first ) ? int( HL_F_NUMBER ) : 0;
	r->num[ 0 ] = w[ 1 ];
	r->num[ 1 ] = hitprint_offset( w, in.slen );
	r->num[ 2 ] = hitprint_len( w, s );
	int32_t	t = r->name_len + 1 + r->score_w;
	t += 3 + rmlist_digits( r->num[ 0 ] ) + rmlist_digits( r->num[ 1 ] ) + rmlist_digits( r->num[ 2 ] );
	for( int c = 0; c < nc; c++ )
		t += 1 + rmlist_field_width( w[ rmlist_field_word( s, HL_FIRST_FIELD + c ) + 1 ] );
	r->temp_len = t + 1;
	return HW_OK;
}

// the bytes of segment g's text in a measured record's lines
RMW_FN int32_t rmlist_seg_len( const HitListRec &r, const int32_t *w, const HitWinShape &s, int g )
{
	switch( g ){
	case HL_NAME : return r.name_len;
	case HL_SCORE : return r.score_w;
	case HL_COMP : case HL_OFFSET : case HL_LEN : return rmlist_digits( rmlist_num( r, g ) );
	default : return rmlist_field_width( w[ rmlist_field_word( s, g ) + 1 ] );
	}
}

// byte j of the joined score fields of a column
RMW_FN uint8_t rmlist_score_byte( const HitListRec &r, const uint8_t *col, int32_t text_len, int32_t j )
{
	if( r.k == 1 )
		return col[ r.tok_at + j ];
	int32_t	pos = 0, at = 0;
	for( int32_t n; ( n = rmlist_token( col, text_len, &pos, &at ) ) > 0; j -= n + 1 )
		if( j <= n )
			return j < n ? col[ at + j ] : uint8_t( ' ' );
	return ' ';
}

// what the bytes of a record are read from
template<class Let> struct HitListView {
	const HitListRec	*r;
	const int32_t	*w;
	const uint8_t	*sid, *col;	// its entry's name, its score column
	int32_t	text_len;
	Let	let;
};

// byte j (0 <= j < rmlist_seg_len) of segment g's text
template<class Let> RMW_FN uint8_t rmlist_seg_byte( const HitListView<Let> &v, const HitWinShape &s, int g, int32_t j )
{
	switch( g ){
	case HL_NAME : return v.sid[ v.r->name_at + j ];
	case HL_SCORE : return rmlist_score_byte( *v.r, v.col, v.text_len, j );
	case HL_COMP : case HL_OFFSET : case HL_LEN : return rmlist_digit_byte( rmlist_num( *v.r, g ), j );
	default : break;
	}
	const int	x = rmlist_field_word( s, g );
	return rmlist_field_byte( v.w[ x ], v.w[ x + 1 ], j, v.let );
}

// byte b (0 <= b < r->temp_len) of the temp line
template<class Let> RMW_FN uint8_t rmlist_temp_byte( const HitListView<Let> &v, const HitWinShape &s, int32_t b )
{
	const int	n = rmlist_n_segs( s );
	for( int g = 0; g < n; g++ ){
		if( g > 0 ){
			if( b == 0 )
				return ' ';
			b--;
		}
		const int32_t	m = rmlist_seg_len( *v.r, v.w, s, g );
		if( b < m )
			return rmlist_seg_byte( v, s, g, b );
		b -= m;
	}
	return '\n';
}

// byte j (0 <= j < width) of a cell of `width` bytes that holds segment g's text of m bytes
template<class Let> RMW_FN uint8_t rmlist_cell_byte( const HitListView<Let> &v, const HitWinShape &s, int g, int32_t m, int32_t width, bool right, int32_t j )
{
	const int32_t	k = right ? j - ( width - m ) : j;
	return k >= 0 && k < m ? rmlist_seg_byte( v, s, g, k ) : uint8_t( ' ' );
}

// the segment byte b (0 <= b < line_len - 1) of a line lies in or, when it is the blank in front of one, behind
RMW_FN int rmlist_find_seg( const int32_t *off, int n, int32_t b )
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

// byte b (0 <= b < l.line_len) of a measured record's line in a listing of layout l
template<class Let> RMW_FN uint8_t rmlist_line_byte( const HitListView<Let> &v, const HitWinShape &s, const HitListLayout &l, int32_t b )
{
	if( b >= l.line_len - 1 )
		return '\n';
	const int	g = rmlist_find_seg( l.off, l.n_segs, b );
	return rmlist_cell_byte( v, s, g, rmlist_seg_len( *v.r, v.w, s, g ), l.width[ g ], l.right[ g ] != 0, b - l.off[ g ] );
}

// The layout of a listing whose segments have these widths (name, score, comp, offset, len, the fields), of records of
// k score fields; right: hitalign_directions' of the program.
inline HitListLayout rmlist_layout( const HitWinShape &s, const uint8_t *right, const int32_t *widths, int32_t k )
{
	HitListLayout	l;
	l.n_segs = rmlist_n_segs( s );
	l.k = k;
	int32_t	at = 0;
	for( int g = 0; g < HL_MAX_SEGS; g++ ){
		l.width[ g ] = g < l.n_segs ? widths[ g ] : 0;
		l.right[ g ] = g == HL_NAME ? 0 : g == HL_SCORE ? ( k == 1 ? 1 : 0 ) : g < HL_FIRST_FIELD ? 1 : right[ g - HL_FIRST_FIELD ];
		if( g > 0 && g < l.n_segs )
			at++;
		l.off[ g ] = at;
		at += l.width[ g ];
	}
	l.line_len = at + 1;
	return l;
}

// -1, 0, 1: two pieces of two temp lines, of la and lb bytes, that stand at the same place of lines equal up to there;
// last: the lines end behind them, else a blank follows -- which no piece holds, so the longer piece's next byte
// decides against it
template<class A, class B> RMW_FN int rmlist_piece_cmp( int32_t la, int32_t lb, bool last, const A &a, const B &b )
{
	const int32_t	m = la < lb ? la : lb;
	for( int32_t j = 0; j < m; j++ ){
		const uint8_t	x = a( j ), y = b( j );
		if( x != y )
			return x < y ? -1 : 1;
	}
	if( la == lb )
		return 0;
	if( last )
		return la < lb ? -1 : 1;
	return la < lb ? ( ' ' < b( m ) ? -1 : 1 ) : ( a( m ) < ' ' ? -1 : 1 );
}

// sort's last resort for two records whose names and numbers are equal: their temp lines by bytes, the shorter first
// where it begins the longer.  What is left to differ are the score fields and the fields.
template<class Let> RMW_FN int rmlist_temp_cmp( const HitListView<Let> &a, const HitListView<Let> &b, const HitWinShape &s )
{
	int32_t	pa = 0, pb = 0, aa = 0, ab = 0;
	for( int32_t t = 0; t < a.r->k; t++ ){
		const int32_t	la = rmlist_token( a.col, a.text_len, &pa, &aa ), lb = rmlist_token( b.col, b.text_len, &pb, &ab );
		const uint8_t	*ca = a.col + aa, *cb = b.col + ab;
		const int	c = rmlist_piece_cmp( la, lb, false, [ ca ]( int32_t j ){ return ca[ j ]; }, [ cb ]( int32_t j ){ return cb[ j ]; } );
		if( c != 0 )
			return c;
	}
	const int	n = rmlist_n_segs( s );
	for( int g = HL_FIRST_FIELD; g < n; g++ ){
		const int	x = rmlist_field_word( s, g );
		const int32_t	oa = a.w[ x ], na = a.w[ x + 1 ], ob = b.w[ x ], nb = b.w[ x + 1 ];
		const int	c = rmlist_piece_cmp( rmlist_field_width( na ), rmlist_field_width( nb ), g == n - 1,
			[ & ]( int32_t j ){ return rmlist_field_byte( oa, na, j, a.let ); }, [ & ]( int32_t j ){ return rmlist_field_byte( ob, nb, j, b.let ); } );
		if( c != 0 )
			return c;
	}
	return 0;
}

// The order of a listing of mode 1 or 2 (every record of the same k; mode 1: k is 1): a before b.  ia, ib: their
// indices in the input, which decide between records whose lines are the same bytes.
template<class Let> RMW_FN bool rmlist_less( int mode, const HitWinShape &s, const HitListView<Let> &a, int64_t ia, const HitListView<Let> &b, int64_t ib )
{
	if( mode == 1 ){
		// -k 2rn,2: descending
		const int	c = rmlist_number_cmp( a.col + a.r->tok_at, a.r->score_w, b.col + b.r->tok_at, b.r->score_w );
		if( c != 0 )
			return c > 0;
	}
	const int32_t	m = a.r->name_len < b.r->name_len ? a.r->name_len : b.r->name_len;
	for( int32_t j = 0; j < m; j++ ){
		const uint8_t	x = a.sid[ a.r->name_at + j ], y = b.sid[ b.r->name_at + j ];
		if( x != y )
			return x < y;
	}
	if( a.r->name_len != b.r->name_len )
		return a.r->name_len < b.r->name_len;
	if( a.r->num[ 0 ] != b.r->num[ 0 ] )
		return a.r->num[ 0 ] < b.r->num[ 0 ];
	if( a.r->num[ 1 ] != b.r->num[ 1 ] )
		return a.r->num[ 1 ] < b.r->num[ 1 ];
	if( a.r->num[ 2 ] != b.r->num[ 2 ] )
		return a.r->num[ 2 ] < b.r->num[ 2 ];
	const int	c = rmlist_temp_cmp( a, b, s );
	return c != 0 ? c < 0 : ia < ib;
}

#if !defined( __HIP_DEVICE_COMPILE__ )
// the words of a refusal by one of the codes above
inline void rmlist_refusal( char *err, size_t errlen, const char *who, int code, long long h )
{
	switch( code ){
	case HL_EMPTY :
		snprintf( err, errlen, "%s: record %lld: an empty score column: rmfmt's listing of it depends on the line read before it (a stale sfields[ 0 ]); "
			"bin/rmfmt resolves that in its own way and this call does not restate it: nothing listed", who, h );
		break;
	case HL_NEWLINE :
		snprintf( err, errlen, "%s: record %lld: a newline in its score column: nothing listed", who, h );
		break;
	case HL_FIELDS :
		snprintf( err, errlen, "%s: record %lld: a line of more than %d fields (MAXFIELDS): nothing listed", who, h, int( HL_MAXFIELDS ) );
		break;
	default :
		snprintf( err, errlen, "%s: record %lld: a hit line of %d bytes or more (LINE_SIZE): nothing listed", who, h, int( HL_LINE_SIZE ) );
		break;
	}
}

// ... and of records whose numbers of score fields differ
inline void rmlist_refusal_mixed( char *err, size_t errlen, const char *who, long long ha, int ka, long long hb, int kb )
{
	snprintf( err, errlen, "%s: records %lld and %lld: %d and %d score fields: rmfmt's order of such records depends on the last line read "
		"(n_sfields in its sort command); bin/rmfmt resolves that in its own way and this call does not restate it: nothing listed", who, ha, hb, ka, kb );
}
#endif

}	// namespace rma
