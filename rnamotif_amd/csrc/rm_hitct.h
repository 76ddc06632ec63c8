// rm_hitct.h -- the connect (.ct) record of a hit record: what rm2ct (tools/rm2ct.cpp; rm2ct.c of the reference) makes of
// the two lines rnamotif prints for it, `-t rnamotif` or `-t rnaviz`, as bytes.
//
// One rule for the host (tests/hostsim/hit_ct_check.cpp, the reasons rma_hit_ct() gives for a refusal) and the device
// (the size and fill kernels of rm_hitct_dev.hip).  The tool parses a hit line from its back end; the rule takes the
// same things from the record's words, for record w of a program, of an entry of slen bases named sid, whose score
// column is the text_len bytes rma_score_hits_text() delivers:
//
//   table     made once per call, on the host, from the words of the "#RM descr" line as read_descr() makes it
//             (rm2ct.c:232-297): a word's first two letters give its kind; strands with the same "(tag...)" text are
//             one helix; untagged h5/h3 and p5/p3 pair by nesting.  Per printed field (the columns of rm_hitalign.h:
//             the left context, the elements, the right context) its kind and the field its partner is counted from.
//   nb        the letters of all printed fields; an empty element is printed as "." and has none
//   bn        the number of a base, from 1, over the fields in order
//   pn        getpn() (rm2ct.c:432-471) for base k (from 0) of a field of len letters: 0 for ss; for h5 / h3 the
//             other strand's first base (from 0) + len - k; for p5 / p3 that first base + k -- from 0, as the tool and
//             the reference have it; -1 for a context
//   hn        comp ? off - bn + 1 : off + bn - 1, off being rm_hitprint.h's offset: the base's place in the entry
//   rnamotif  "%4d %s %d %d %d\n" of nb, sid, comp, off, len; per base "%4d %c %4d %4d %4d %4d\n" of bn, the letter,
//             bn - 1, bn + 1 (0 behind the last base), pn, hn
//   rnaviz    "%5d dG = %.3f \"%s %d %d %d\"\n" with the energy in front of the name; per base "%5d %c %7d %4d %4d %4d\n",
//             the letter in upper case
//   energy    float( atof( the hit line behind the name ) ): blanks, an optional sign, digits with an optional point.
//             The value M / 10^k (M below 10^19, k at most 19) is rounded once to double, to nearest even, by integer
//             long division with a sticky bit, then converted to float -- the tool's two roundings.  Nothing to convert
//             is 0.0; a column without a number in front lets the tool read on into " %d" of comp.  A zero keeps its
//             sign.  What is not restated stops the record (HC_NUMBER): strtod's inf, nan, 0x and exponent forms, more
//             than 19 digits from the first one that is not 0 to the last, more than 19 behind the point.
//   letters   rm_hitwin.h's, as rm_hitprint.h reads them; integers through rms_fmt_int, %.3f through rms_fmt_f (a float
//             of 2^63 or more, which rms_fmt_f does not take, is an integer: rms_fmt_u64 and ".000")
//
// Lengths are counted in hitct_line_len() and hitct_size() alone.  A record is checked by hitprint_check before anything
// of it is used, then (hitct_measure) refused where the tool would not see the line rnamotif printed: a newline in the
// score column, a hit line of 50 000 bytes or more (the tool's line buffer) -- so nb stays below 50 000.  The tool
// refuses a descriptor with a triple or quad helix; so does hitct_table().
#pragma once
#include <cstdio>
#include "rm_hitprint.h"

namespace rma {

enum { HC_RNAMOTIF = 0, HC_RNAVIZ = 1 };
enum { HC_K_UNKNOWN = -1, HC_K_CTX, HC_K_SS, HC_K_H5, HC_K_H3, HC_K_P5, HC_K_P3, HC_K_T1, HC_K_T2, HC_K_T3, HC_K_Q1, HC_K_Q2, HC_K_Q3, HC_K_Q4 };
// what refuses a record, behind hitprint_check's codes
enum { HC_NEWLINE = HP_TEXT + 1, HC_LINE, HC_NUMBER };
enum { HC_LINE_SIZE = 50000 };
// room for a base's line (at most 5 + 3 + 7 + 1 + 5 + 1 + 6 + 1 + 11 + 1 = 41 bytes), for a header line in front of
// the name (at most 5 + 6 + 24 + 2) and behind it (at most 3 * 12 + 2), for the prefix of the field lengths
enum { HC_LINE_CAP = 48, HC_HEAD_CAP = 48, HC_TAIL_CAP = 48, HC_PRE_ROOM = 128 };
static_assert( int( HA_MAX_COLS ) < int( HC_PRE_ROOM ), "two lane passes hold the prefix of a record's fields" );

// per printed field: its kind, and the field whose first base its partner is counted from (-1: none)
struct HitCtTable {
	int32_t	n;
	int16_t	mate[ HA_MAX_COLS ];
	int8_t	kind[ HA_MAX_COLS ];
};

// the header line's numbers of a checked record
struct HitCtHead {
	int32_t	nb, comp, off, len;
};

// the letters of printed field c (0 <= c < hitalign_n_cols)
RMW_FN int32_t hitct_field_len( const int32_t *w, const HitWinShape &s, int c )
{
	const int32_t	len = w[ hitstruct_word( s, hitalign_col_elem( s, c ) ) + 1 ];
	return len > 0 ? len : 0;
}

// pre[ c ] = the letters in front of field c, pre[ n ] = nb.  (The kernels lay the same sums into LDS by a wave-wide prefix.)
RMW_FN void hitct_prefix( const int32_t *w, const HitWinShape &s, int32_t *pre )
{
	const int	n = hitalign_n_cols( s );
	pre[ 0 ] = 0;
	for( int c = 0; c < n; c++ )
		pre[ c + 1 ] = pre[ c ] + hitct_field_len( w, s, c );
}

// the field base bn lies in: the last c of n with pre[ c ] < bn (an empty field has no base: the one behind it wins)
RMW_FN int hitct_find_field( const int32_t *pre, int n, int32_t bn )
{
	int	lo = 0, hi = n - 1;
	while( lo < hi ){
		const int	mid = ( lo + hi + 1 ) >> 1;
		if( pre[ mid ] < bn )
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

// getpn(): the partner of base k of field c
RMW_FN int32_t hitct_partner( const int8_t *kind, const int16_t *mate, const int32_t *pre, int c, int32_t k )
{
	const int32_t	len = pre[ c + 1 ] - pre[ c ];
	switch( kind[ c ] ){
	case HC_K_SS : return 0;
	case HC_K_H5 : case HC_K_H3 : return pre[ mate[ c ] ] + len - k;
	case HC_K_P5 : case HC_K_P3 : return pre[ mate[ c ] ] + k;
	case HC_K_CTX : case HC_K_UNKNOWN : return -1;
	default : return 0;
	}
}

// (the tool's ints; they wrap where a record somebody made by hand overflows them)
RMW_FN int32_t hitct_hn( const HitCtHead &h, int32_t bn )
{
	return int32_t( h.comp ? uint32_t( h.off ) - uint32_t( bn ) + 1u : uint32_t( h.off ) + uint32_t( bn ) - 1u );
}

RMW_FN HitCtHead hitct_head_of( const int32_t *w, const HitWinShape &s, int32_t slen, int32_t nb )
{
	return HitCtHead{ nb, w[ 1 ], hitprint_offset( w, slen ), hitprint_len( w, s ) };
}

// the line of base bn whose letter, partner and place are given, into buf[ cap ]; returns its length (cap 0: the length alone)
RMW_FN int hitct_line( int type, int32_t bn, int32_t nb, uint8_t letter, int32_t pn, int32_t hn, uint8_t *buf, int cap )
{
	RmsSink	o{ buf, 1, 0, cap, 0 };
	rms_fmt_int( o, RmsSpec{ 0, type == HC_RNAVIZ ? 5 : 4, -1 }, 'd', bn );
	o.put( ' ' );
	o.put( type == HC_RNAVIZ && letter >= 'a' && letter <= 'z' ? uint8_t( letter - ( 'a' - 'A' ) ) : letter );
	o.put( ' ' );
	rms_fmt_int( o, RmsSpec{ 0, type == HC_RNAVIZ ? 7 : 4, -1 }, 'd', bn - 1 );
	o.put( ' ' );
	rms_fmt_int( o, RmsSpec{ 0, 4, -1 }, 'd', bn == nb ? 0 : bn + 1 );
	o.put( ' ' );
	rms_fmt_int( o, RmsSpec{ 0, 4, -1 }, 'd', pn );
	o.put( ' ' );
	rms_fmt_int( o, RmsSpec{ 0, 4, -1 }, 'd', hn );
	o.put( '\n' );
	return o.n;
}

// Base bn (1 <= bn <= h.nb) of a record: *c its field, *k its index there, *pn its partner; returns hn
RMW_FN int32_t hitct_base( const int8_t *kind, const int16_t *mate, const int32_t *pre, int n, const HitCtHead &h, int32_t bn, int *c, int32_t *k, int32_t *pn )
{
	*c = hitct_find_field( pre, n, bn );
	*k = bn - 1 - pre[ *c ];
	*pn = hitct_partner( kind, mate, pre, *c, *k );
	return hitct_hn( h, bn );
}

// the bytes of base bn's line
RMW_FN int hitct_line_len( int32_t bn, int type, const int8_t *kind, const int16_t *mate, const int32_t *pre, int n, const HitCtHead &h )
{
	int	c;
	int32_t	k, pn;
	const int32_t	hn = hitct_base( kind, mate, pre, n, h, bn, &c, &k, &pn );
	return hitct_line( type, bn, h.nb, 'n', pn, hn, nullptr, 0 );
}

// %.3f of an energy: rms_fmt_f's, which stops at 2^63; a float from there to the 10^19 the digits end below is an
// integer of 64 bits
RMW_FN void hitct_fmt_energy( RmsSink &o, float energy )
{
	const float	a = energy < 0 ? -energy : energy;
	if( a >= 9223372036854775808.0f ){
		if( energy < 0 )
			o.put( '-' );
		rms_fmt_u64( o, uint64_t( a ) );
		o.put( '.' );
		o.fill( '0', 3 );
	}else
		rms_fmt_f( o, RmsSpec{ 0, 0, 3 }, double( energy ) );
}

// the header line in front of the name ...
RMW_FN int hitct_head( int type, const HitCtHead &h, float energy, uint8_t *buf, int cap )
{
	RmsSink	o{ buf, 1, 0, cap, 0 };
	rms_fmt_int( o, RmsSpec{ 0, type == HC_RNAVIZ ? 5 : 4, -1 }, 'd', h.nb );
	o.put( ' ' );
	if( type == HC_RNAVIZ ){
		const char	*dg = "dG = ";
		for( int i = 0; dg[ i ]; i++ )
			o.put( uint8_t( dg[ i ] ) );
		hitct_fmt_energy( o, energy );
		o.put( ' ' );
		o.put( '"' );
	}
	return o.n;
}

// ... and behind it
RMW_FN int hitct_tail( int type, const HitCtHead &h, uint8_t *buf, int cap )
{
	RmsSink	o{ buf, 1, 0, cap, 0 };
	o.put( ' ' );
	rms_fmt_int( o, RmsSpec{ 0, 0, -1 }, 'd', h.comp );
	o.put( ' ' );
	rms_fmt_int( o, RmsSpec{ 0, 0, -1 }, 'd', h.off );
	o.put( ' ' );
	rms_fmt_int( o, RmsSpec{ 0, 0, -1 }, 'd', h.len );
	if( type == HC_RNAVIZ )
		o.put( '"' );
	o.put( '\n' );
	return o.n;
}

// The bytes of every step-th line of a record from line `first` on, line 0 being the header line, line bn base bn's:
// first 0, step 1 is the record (hitct_size); lane l of a wave takes first l, step 64, and the wave adds them up.
RMW_FN int64_t hitct_size_part( int type, const int8_t *kind, const int16_t *mate, const int32_t *pre, int n, const HitCtHead &h, float energy,
	int64_t sid_len, int32_t first, int32_t step )
{
	int64_t	size = 0;
	if( first == 0 )
		size = hitct_head( type, h, energy, nullptr, 0 ) + sid_len + hitct_tail( type, h, nullptr, 0 );
	for( int32_t bn = first == 0 ? step : first; bn <= h.nb; bn += step )
		size += hitct_line_len( bn, type, kind, mate, pre, n, h );
	return size;
}

// the bytes of a measured record; 0 for a record that is not accepted
RMW_FN int64_t hitct_size( int type, const HitCtTable &t, const int32_t *pre, const HitCtHead &h, float energy, int64_t sid_len, bool accept )
{
	return accept ? hitct_size_part( type, t.kind, t.mate, pre, t.n, h, energy, sid_len, 0, 1 ) : 0;
}

// Byte j of the hit line rnamotif prints for the record, counted from the byte behind the name: hitprint_byte() of the
// byte behind the definition line and the name, taken up at the segment there.  src as hitprint_seg_byte takes it.
template<class Src> RMW_FN uint8_t hitct_behind_name( const int32_t *w, const HitWinShape &s, const HitPrintIn &in, int num_len, int64_t j, const Src &src )
{
	const int	n = hitprint_n_segs( s );
	for( int k = 6; k < n; k++ ){
		const HitPrintSeg	g = hitprint_seg( w, s, in, num_len, k );
		if( j < g.len )
			return hitprint_seg_byte( w, g, j, src );
		j -= g.len;
	}
	return 0;
}

RMW_FN bool hitct_space( uint8_t c )
{
	return c == ' ' || ( c >= '\t' && c <= '\r' );
}

RMW_FN bool hitct_digit( uint8_t c )
{
	return c >= '0' && c <= '9';
}

RMW_FN bool hitct_hex( uint8_t c )
{
	return hitct_digit( c ) || ( ( c | 0x20 ) >= 'a' && ( c | 0x20 ) <= 'f' );
}

// M / 10^k (0 < M < 10^19, k <= 19) as the nearest double, ties to even: long division, bit by bit, the remainder's
// being non-zero the sticky bit
RMW_FN uint64_t hitct_ratio_bits( uint64_t M, int k )
{
	uint64_t	D = 1;
	for( int i = 0; i < k; i++ )
		D *= 10;
	uint64_t	I = M / D, R = M - I * D, mant;
	int	e = 0;
	bool	round, sticky;
	auto next_bit = [ & ]() -> uint64_t {
		// R < D < 2^64: 2 R may not fit, its carry counts
		const bool	carry = ( R >> 63 ) != 0;
		R <<= 1;
		if( carry || R >= D ){
			R -= D;
			return 1;
		}
		return 0;
	};
	if( I >> 53 ){
		int	sh = 0;
		while( ( I >> sh ) >> 53 )
			sh++;
		mant = I >> sh;
		const uint64_t	low = I & ( ( uint64_t( 1 ) << sh ) - 1 ), half = uint64_t( 1 ) << ( sh - 1 );
		round = ( low & half ) != 0;
		sticky = ( low & ( half - 1 ) ) != 0 || R != 0;
		e = sh;
	}else{
		mant = I;
		while( !( mant >> 52 ) ){
			mant = ( mant << 1 ) | next_bit();
			e--;
		}
		round = next_bit() != 0;
		sticky = R != 0;
	}
	if( round && ( sticky || ( mant & 1 ) ) )
		if( ( ++mant >> 53 ) != 0 ){
			mant >>= 1;
			e++;
		}
	return ( uint64_t( e + 52 + 1023 ) << 52 ) | ( mant & ( ( uint64_t( 1 ) << 52 ) - 1 ) );
}

// float( atof() ) of the n bytes get( 0 ) .. get( n - 1 ): HW_OK and *energy, or HC_NUMBER
template<class Get> RMW_FN int hitct_energy( const Get &get, int64_t n, float *energy )
{
	auto at = [ & ]( int64_t i ) -> uint8_t { return i < n ? get( i ) : uint8_t( 0 ); };
	*energy = 0.0f;
	int64_t	i = 0;
	while( hitct_space( at( i ) ) )
		i++;
	bool	neg = false;
	if( at( i ) == '+' || at( i ) == '-' )
		neg = at( i++ ) == '-';
	const uint8_t	a = at( i ) | 0x20, b = at( i + 1 ) | 0x20, c = at( i + 2 ) | 0x20;
	if( ( a == 'i' && b == 'n' && c == 'f' ) || ( a == 'n' && b == 'a' && c == 'n' ) )
		return HC_NUMBER;
	if( at( i ) == '0' && b == 'x' && ( hitct_hex( at( i + 2 ) ) || ( at( i + 2 ) == '.' && hitct_hex( at( i + 3 ) ) ) ) )
		return HC_NUMBER;
	uint64_t	M = 0;
	int	sig = 0, k = 0;
	bool	any = false, point = false;
	for( ; ; i++ ){
		const uint8_t	d = at( i );
		if( hitct_digit( d ) ){
			any = true;
			if( sig > 0 || d != '0' ){
				if( sig == 19 )
					return HC_NUMBER;
				M = M * 10 + uint64_t( d - '0' );
				sig++;
			}
			if( point && ++k > 19 )
				return HC_NUMBER;
		}else if( d == '.' && !point )
			point = true;
		else
			break;
	}
	if( !any )
		return HW_OK;		// nothing converted: 0.0, whatever sign stood there
	if( ( at( i ) | 0x20 ) == 'e' ){
		const int64_t	j = at( i + 1 ) == '+' || at( i + 1 ) == '-' ? i + 2 : i + 1;
		if( hitct_digit( at( j ) ) )
			return HC_NUMBER;
	}
	const uint64_t	bits = ( neg ? uint64_t( 1 ) << 63 : 0 ) | ( M != 0 ? hitct_ratio_bits( M, k ) : 0 );
	double	x;
	memcpy( &x, &bits, sizeof( x ) );
	*energy = float( x );
	return HW_OK;
}

// A record hitprint_check has passed, measured: HW_OK and *energy (0 in rnamotif mode), or what refuses it.  num_len:
// what hitprint_numbers returned, for src.num(); src as hitprint_seg_byte takes it (its letters are not read).
template<class Src> RMW_FN int hitct_measure( const int32_t *w, const HitWinShape &s, const HitPrintIn &in, int type, int num_len, const Src &src,
	float *energy )
{
	*energy = 0.0f;
	for( int32_t i = 0; i < in.text_len; i++ )
		if( src.score( i ) == '\n' )
			return HC_NEWLINE;
	// the hit line as rnamotif prints it: the record's two lines without the definition line
	const int64_t	line = hitprint_size( w, s, in, true ) - ( 3 + in.sid_len + in.sdef_len );
	if( line >= HC_LINE_SIZE )
		return HC_LINE;
	if( type != HC_RNAVIZ )
		return HW_OK;
	return hitct_energy( [ & ]( int64_t j ){ return hitct_behind_name( w, s, in, num_len, j, src ); }, line - in.sid_len, energy );
}

// Byte b (0 <= b < hitct_size) of a measured record, for the host: the lines in turn.
template<class Src> inline uint8_t hitct_byte( int type, const HitCtTable &t, const int32_t *w, const HitWinShape &s, const int32_t *pre, const HitCtHead &h,
	float energy, int64_t sid_len, int64_t b, const Src &src )
{
	uint8_t	buf[ HC_LINE_CAP ];
	const int	hl = hitct_head( type, h, energy, buf, HC_HEAD_CAP );
	if( b < hl )
		return buf[ b ];
	b -= hl;
	if( b < sid_len )
		return src.sid( b );
	b -= sid_len;
	const int	tl = hitct_tail( type, h, buf, HC_TAIL_CAP );
	if( b < tl )
		return buf[ b ];
	b -= tl;
	for( int32_t bn = 1; bn <= h.nb; bn++ ){
		int	c;
		int32_t	k, pn;
		const int32_t	hn = hitct_base( t.kind, t.mate, pre, t.n, h, bn, &c, &k, &pn );
		const int	m = hitct_line( type, bn, h.nb, 'n', pn, hn, nullptr, 0 );
		if( b < m ){
			const uint8_t	letter = src.letter( w[ hitstruct_word( s, hitalign_col_elem( s, c ) ) ] + k );
			hitct_line( type, bn, h.nb, letter, pn, hn, buf, HC_LINE_CAP );
			return buf[ b ];
		}
		b -= m;
	}
	return 0;
}

#if !defined( __HIP_DEVICE_COMPILE__ )
// The table of a descriptor whose "#RM descr" line has these words behind "#RM descr" (rma_descr_names), for a program of
// n_cols printed fields.  0, or 1 with the tool's words for a triple or quad helix and words of its own for a line the
// tool would index out of its table with.
inline int hitct_table( const char *words, int n_cols, HitCtTable *t, char *err, size_t errlen )
{
	const char	*names[] = { "ctx", "ss", "h5", "h3", "p5", "p3", "t1", "t2", "t3", "q1", "q2", "q3", "q4" };
	// the words, split as the tool splits them
	const char	*at[ HA_MAX_COLS ];
	size_t	len[ HA_MAX_COLS ];
	int	n = 0;
	for( const char *p = words != nullptr ? words : ""; *p; ){
		while( *p == ' ' || *p == '\t' || *p == '\n' )
			p++;
		const char	*q = p;
		while( *q && *q != ' ' && *q != '\t' && *q != '\n' )
			q++;
		if( q > p ){
			if( n < HA_MAX_COLS ){
				at[ n ] = p;
				len[ n ] = size_t( q - p );
			}
			n++;
		}
		p = q;
	}
	if( n != n_cols || n > HA_MAX_COLS ){
		snprintf( err, errlen, "the \"#RM descr\" line has %d words, the program prints %d fields (a tag with a blank in it?): rm2ct would take the wrong fields", n, n_cols );
		return 1;
	}
	int	group[ HA_MAX_COLS ][ 4 ];
	auto tag_of = [ & ]( int d, size_t *m ) -> const char * {
		const char	*p = static_cast<const char *>( memchr( at[ d ], '(', len[ d ] ) );
		*m = p != nullptr ? len[ d ] - size_t( p - at[ d ] ) : 0;
		return p;
	};
	t->n = n;
	for( int d = 0; d < HA_MAX_COLS; d++ ){
		t->kind[ d ] = HC_K_UNKNOWN;
		t->mate[ d ] = -1;
		for( int m = 0; m < 4; m++ )
			group[ d ][ m ] = -1;
		if( d >= n )
			continue;
		for( int k = 0; k < 13; k++ )
			if( len[ d ] >= 2 && names[ k ][ 0 ] == at[ d ][ 0 ] && names[ k ][ 1 ] == at[ d ][ 1 ] ){
				t->kind[ d ] = int8_t( k );
				break;
			}
	}
	for( int d = 0; d < n; d++ )
		if( t->kind[ d ] == HC_K_T1 || t->kind[ d ] == HC_K_Q1 ){
			snprintf( err, errlen, "can't make CT file for %s helices.", t->kind[ d ] == HC_K_T1 ? "triple" : "quad" );
			return 1;
		}
	// tagged strands: the same "(tag)" text
	for( int d = 0; d < n; d++ ){
		size_t	m, m1;
		const char	*tag = tag_of( d, &m );
		if( t->kind[ d ] == HC_K_SS || tag == nullptr || group[ d ][ 0 ] != -1 )
			continue;
		int	k = 0;
		group[ d ][ k++ ] = d;
		for( int d1 = d + 1; d1 < n; d1++ ){
			const char	*tag1 = tag_of( d1, &m1 );
			if( tag1 != nullptr && m1 == m && !memcmp( tag1, tag, m ) && k < 4 )
				group[ d ][ k++ ] = d1;
		}
		for( int j = 1; j < 4 && group[ d ][ j ] != -1; j++ )
			memcpy( group[ group[ d ][ j ] ], group[ d ], sizeof( group[ d ] ) );
	}
	// untagged duplexes pair by nesting
	int	stk[ HA_MAX_COLS ], sp = 0;
	for( int d = 0; d < n; d++ ){
		if( t->kind[ d ] == HC_K_SS || group[ d ][ 0 ] != -1 )
			continue;
		if( t->kind[ d ] == HC_K_H5 || t->kind[ d ] == HC_K_P5 )
			stk[ sp++ ] = d;
		else if( ( t->kind[ d ] == HC_K_H3 || t->kind[ d ] == HC_K_P3 ) && sp > 0 ){
			const int	d5 = stk[ --sp ];
			group[ d5 ][ 0 ] = group[ d ][ 0 ] = d5;
			group[ d5 ][ 1 ] = group[ d ][ 1 ] = d;
		}
	}
	for( int d = 0; d < n; d++ ){
		const int	kd = t->kind[ d ];
		if( kd != HC_K_H5 && kd != HC_K_H3 && kd != HC_K_P5 && kd != HC_K_P3 )
			continue;
		const int	m = group[ d ][ kd == HC_K_H5 || kd == HC_K_P5 ? 1 : 0 ];
		if( m < 0 ){
			snprintf( err, errlen, "field %d of the \"#RM descr\" line is a strand without a partner: rm2ct would read outside its table", d );
			return 1;
		}
		t->mate[ d ] = int16_t( m );
	}
	return 0;
}

// the words of a refusal by one of the codes above
inline void hitct_refusal( char *err, size_t errlen, const char *who, int code, long long h )
{
	switch( code ){
	case HC_NEWLINE :
		snprintf( err, errlen, "%s: record %lld: a newline in its score column: nothing written", who, h );
		break;
	case HC_LINE :
		snprintf( err, errlen, "%s: record %lld: a hit line of %d bytes or more (rm2ct's line buffer): nothing written", who, h, int( HC_LINE_SIZE ) );
		break;
	default :
		snprintf( err, errlen, "%s: record %lld: the text behind its name is an inf, nan, 0x or exponent form of strtod's, has more than 19 digits from its first "
			"non-zero digit to its last or behind the point: rm2ct -t rnaviz reads it with atof(), which this call does not restate (HC_NUMBER): nothing written", who, h );
		break;
	}
}
#endif

}	// namespace rma
