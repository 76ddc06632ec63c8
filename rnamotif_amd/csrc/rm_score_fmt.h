// rm_score_fmt.h -- printf's %d %i %u %o %x %X, %s and %f as the rule of rm_score_core.h writes them, for the host and
// the device alike: the bytes glibc's snprintf gives, made without a buffer, without a table of digits and without float
// arithmetic.  sprintf() of the score section and the score column of a hit (" %8d", " %8.3lf", " %8s" of
// HitPrinter::print) both go through these.
//
// A directive is its flags (- + blank 0 #), a width and a precision (RmsSpec; rms_fmt_parse reads them from the bytes
// between '%' and the conversion letter and refuses anything else: '*', '$', a length modifier, the ' and I flags).
// Bytes go to a sink (RmsSink): byte k of a lane's arena lies at ( k >> 2 ) * 4 * S + ( k & 3 ) -- S 1 is a plain
// array, S 64 the dwords of a wave's 64 lanes interleaved.  A sink counts past its end without writing, so that a
// string that does not fit is known by its length.
//
// %f is exact for every finite double with |x| < 2^63 and a precision of at most 18: the integer part is a 64-bit
// integer, the fraction a fixed-point number of 128 bits (and one sticky bit for what a subnormal has below them),
// multiplied by ten once per digit; the digits behind the point are gathered in a 64-bit integer (18 digits fit), the
// rest decides the rounding -- to nearest on the exact binary value, ties to even, as glibc rounds in the default
// mode -- and a carry runs into the integer part.  The sign is the sign bit's: -0.0004 is "-0.000".
#pragma once
#include <cstdint>
#include <cstring>

#ifndef RMD_FN
#define RMD_FN	static inline
#endif
#ifndef RMD_FN_MEMBER
#define RMD_FN_MEMBER	inline
#endif

enum { RMS_FL_MINUS = 1, RMS_FL_PLUS = 2, RMS_FL_SPACE = 4, RMS_FL_ZERO = 8, RMS_FL_ALT = 16 };
enum { RMS_FMT_OK, RMS_FMT_PREC, RMS_FMT_RANGE };
enum { RMS_FMT_MAX_PREC = 18, RMS_FMT_MAX_NUMBER = 1 << 24 };

struct RmsSpec {
	int	flags, width, prec;	// prec -1: none given
};

struct RmsSink {
	uint8_t	*p;
	int	S;		// the arena's interleave
	int	base, cap;	// the first byte written, the arena's end
	int	n;		// bytes put, written or not
	RMD_FN_MEMBER void	put( unsigned char c )
	{
		const int	k = base + n;
		if( k >= 0 && k < cap )
			p[ ( k >> 2 ) * 4 * S + ( k & 3 ) ] = c;
		n++;
	}
	RMD_FN_MEMBER void	fill( unsigned char c, int k )
	{
		for( ; k > 0 && base + n < cap; k-- )
			put( c );
		if( k > 0 )
			n = k > RMS_FMT_MAX_NUMBER - n ? RMS_FMT_MAX_NUMBER : n + k;
	}
};

// the conversion letters do_sprintf's strpbrk() stops at
RMD_FN int rms_fmt_is_conv( unsigned char c )
{
	switch( c ){
	case 'b' : case 'B' : case 'd' : case 'i' : case 'o' : case 'u' : case 'x' : case 'X' : case 'f' : case 'e' : case 'E' : case 'g' : case 'G' :
	case 'c' : case 'C' : case 's' : case 'S' : case 'p' : case 'n' : case '%' :
		return 1;
	default :
		return 0;
	}
}

// flags, width and precision of the bytes get( from ) .. get( to - 1 ) of a directive; 0: there is something else
template< class Get > RMD_FN int rms_fmt_parse( const Get &get, int from, int to, RmsSpec *sp )
{
	int	i = from;
	sp->flags = 0;
	sp->width = 0;
	sp->prec = -1;
	for( ; i < to; i++ ){
		const unsigned char	c = get( i );
		if( c == '-' ) sp->flags |= RMS_FL_MINUS;
		else if( c == '+' ) sp->flags |= RMS_FL_PLUS;
		else if( c == ' ' ) sp->flags |= RMS_FL_SPACE;
		else if( c == '0' ) sp->flags |= RMS_FL_ZERO;
		else if( c == '#' ) sp->flags |= RMS_FL_ALT;
		else break;
	}
	for( ; i < to; i++ ){
		const unsigned char	c = get( i );
		if( c < '0' || c > '9' )
			break;
		sp->width = sp->width >= RMS_FMT_MAX_NUMBER ? RMS_FMT_MAX_NUMBER : sp->width * 10 + ( c - '0' );
	}
	if( i < to && get( i ) == '.' ){
		sp->prec = 0;
		for( i++; i < to; i++ ){
			const unsigned char	c = get( i );
			if( c < '0' || c > '9' )
				break;
			sp->prec = sp->prec >= RMS_FMT_MAX_NUMBER ? RMS_FMT_MAX_NUMBER : sp->prec * 10 + ( c - '0' );
		}
	}
	return i == to;
}

// sign or prefix, zeros and digits between the padding a width asks for
RMD_FN void rms_fmt_pad_left( RmsSink &o, const RmsSpec &sp, int body, bool zero_ok, int *zeros )
{
	const int	pad = sp.width > body ? sp.width - body : 0;
	if( sp.flags & RMS_FL_MINUS )
		;
	else if( ( sp.flags & RMS_FL_ZERO ) && zero_ok )
		*zeros += pad;
	else
		o.fill( ' ', pad );
}
RMD_FN void rms_fmt_pad_right( RmsSink &o, const RmsSpec &sp, int body )
{
	if( ( sp.flags & RMS_FL_MINUS ) && sp.width > body )
		o.fill( ' ', sp.width - body );
}

RMD_FN void rms_fmt_u64( RmsSink &o, uint64_t v )
{
	uint64_t	p = 1;
	while( v / p >= 10 )
		p *= 10;
	for( ; p > 0; p /= 10 ){
		const uint64_t	d = v / p;
		o.put( static_cast<unsigned char>( '0' + d ) );
		v -= d * p;
	}
}

// %d %i %u %o %x %X of an int
RMD_FN void rms_fmt_int( RmsSink &o, const RmsSpec &sp, unsigned char conv, int32_t v )
{
	const bool	is_signed = conv == 'd' || conv == 'i', neg = is_signed && v < 0;
	const uint32_t	u = neg ? 0u - uint32_t( v ) : uint32_t( v );
	const uint32_t	base = conv == 'o' ? 8u : conv == 'x' || conv == 'X' ? 16u : 10u;
	int	nd = 0;
	for( uint32_t t = u; t != 0; t /= base )
		nd++;
	int	mind = sp.prec < 0 ? 1 : sp.prec;
	if( ( sp.flags & RMS_FL_ALT ) && base == 8u && mind <= nd )
		mind = nd + 1;
	int	zeros = mind > nd ? mind - nd : 0;
	const unsigned char	sign = neg ? '-' : !is_signed ? 0 : ( sp.flags & RMS_FL_PLUS ) ? '+' : ( sp.flags & RMS_FL_SPACE ) ? ' ' : 0;
	const bool	prefix = ( sp.flags & RMS_FL_ALT ) && base == 16u && u != 0;
	const int	body = ( sign ? 1 : 0 ) + ( prefix ? 2 : 0 ) + zeros + nd;
	rms_fmt_pad_left( o, sp, body, sp.prec < 0, &zeros );
	if( sign )
		o.put( sign );
	if( prefix ){
		o.put( '0' );
		o.put( conv );
	}
	o.fill( '0', zeros );
	if( nd > 0 ){
		uint32_t	p = 1, t = u;
		for( int i = 1; i < nd; i++ )
			p *= base;
		for( ; p > 0; p /= base ){
			const uint32_t	d = t / p;
			o.put( static_cast<unsigned char>( d < 10 ? '0' + d : ( conv == 'X' ? 'A' : 'a' ) + ( d - 10 ) ) );
			t -= d * p;
		}
	}
	rms_fmt_pad_right( o, sp, body );
}

// %s of the len bytes get( 0 ) .. get( len - 1 )
template< class Get > RMD_FN void rms_fmt_str( RmsSink &o, const RmsSpec &sp, const Get &get, int len )
{
	const int	n = sp.prec >= 0 && sp.prec < len ? sp.prec : len;
	if( !( sp.flags & RMS_FL_MINUS ) && sp.width > n )
		o.fill( ' ', sp.width - n );
	for( int i = 0; i < n; i++ )
		o.put( get( i ) );
	rms_fmt_pad_right( o, sp, n );
}

// %f of a double; RMS_FMT_PREC: a precision above 18, RMS_FMT_RANGE: not finite or |x| >= 2^63 -- nothing is put then
RMD_FN int rms_fmt_f( RmsSink &o, const RmsSpec &sp, double x )
{
	uint64_t	u;
	memcpy( &u, &x, sizeof( u ) );
	const bool	neg = ( u >> 63 ) != 0;
	const int	ex = int( ( u >> 52 ) & 0x7ff );
	const uint64_t	man = u & ( ( uint64_t( 1 ) << 52 ) - 1 );
	const int	P = sp.prec < 0 ? 6 : sp.prec;
	if( ex == 0x7ff )
		return RMS_FMT_RANGE;
	const uint64_t	m = ex == 0 ? man : man | ( uint64_t( 1 ) << 52 );
	const int	e = ex == 0 ? -1074 : ex - 1075;		// |x| = m * 2^e
	if( m != 0 && e > 10 )
		return RMS_FMT_RANGE;
	if( P > RMS_FMT_MAX_PREC )
		return RMS_FMT_PREC;
	uint64_t	I = 0, fh = 0, fl = 0;
	bool	sticky = false;
	if( m == 0 )
		;
	else if( e >= 0 )
		I = m << e;
	else{
		const int	s = -e;
		if( s < 64 ){
			I = m >> s;
			fh = ( m & ( ( uint64_t( 1 ) << s ) - 1 ) ) << ( 64 - s );
		}else if( s == 64 )
			fh = m;
		else if( s < 128 ){
			fh = m >> ( s - 64 );
			fl = m << ( 128 - s );
		}else if( s - 128 < 64 ){
			fl = m >> ( s - 128 );
			sticky = ( m & ( ( uint64_t( 1 ) << ( s - 128 ) ) - 1 ) ) != 0;
		}else
			sticky = true;
	}
	// the fraction's 128 bits as four limbs; times ten per digit, the digit is what leaves at the top
	uint64_t	f3 = fh >> 32, f2 = fh & 0xffffffffu, f1 = fl >> 32, f0 = fl & 0xffffffffu, Fd = 0, ten_P = 1;
	for( int i = 0; i < P; i++ ){
		uint64_t	t = f0 * 10;
		f0 = t & 0xffffffffu;
		t = f1 * 10 + ( t >> 32 );
		f1 = t & 0xffffffffu;
		t = f2 * 10 + ( t >> 32 );
		f2 = t & 0xffffffffu;
		t = f3 * 10 + ( t >> 32 );
		f3 = t & 0xffffffffu;
		Fd = Fd * 10 + ( t >> 32 );
		ten_P *= 10;
	}
	const bool	low = ( f2 | f1 | f0 ) != 0 || sticky;
	const bool	above = f3 > 0x80000000u || ( f3 == 0x80000000u && low ), tie = f3 == 0x80000000u && !low;
	if( above || ( tie && ( ( P > 0 ? Fd : I ) & 1 ) ) ){
		if( ++Fd == ten_P ){
			Fd = 0;
			I++;
		}
	}
	int	nd = 1, zeros = 0;
	for( uint64_t t = I; t >= 10; t /= 10 )
		nd++;
	const unsigned char	sign = neg ? '-' : ( sp.flags & RMS_FL_PLUS ) ? '+' : ( sp.flags & RMS_FL_SPACE ) ? ' ' : 0;
	const bool	dot = P > 0 || ( sp.flags & RMS_FL_ALT );
	const int	body = ( sign ? 1 : 0 ) + nd + ( dot ? 1 : 0 ) + P;
	rms_fmt_pad_left( o, sp, body, true, &zeros );
	if( sign )
		o.put( sign );
	o.fill( '0', zeros );
	rms_fmt_u64( o, I );
	if( dot )
		o.put( '.' );
	for( uint64_t p = ten_P / 10; p > 0; p /= 10 ){
		const uint64_t	d = Fd / p;
		o.put( static_cast<unsigned char>( '0' + d ) );
		Fd -= d * p;
	}
	rms_fmt_pad_right( o, sp, body );
	return RMS_FMT_OK;
}
