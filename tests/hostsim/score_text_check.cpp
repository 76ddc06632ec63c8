// score_text_check.cpp -- the rule of rnamotif_amd/csrc/rm_score_core.h for an image with text (sprintf(), bits(),
// string +, a string in SCORE) and the formatter of rm_score_fmt.h, on the host.
//
//   score_text_check fmt SEED COUNT
// The formatter alone against snprintf: COUNT doubles of eight generators seeded with SEED, SEED + 1 ... -- random bit patterns, fractions
// of every scale, exact ties, subnormals -- each written with every precision from 0 to 18 under flag and width
// combinations that change from value to value; then negative zero, values just under 2^63, ties at every precision,
// float( 0.01 * k ) for every energy word k in [ -20000, 20000 ] at every precision; %d %i %u %o %x %X and %s under
// every combination of flags, widths and precisions.  Inside the domain the bytes must be equal; outside it -- not
// finite, 2^63 or more, a precision above 18 -- the formatter must refuse.  Prints "FMT checked=<n> refused=<n> bad=<n>"
// and the first disagreements; status 1 if there is one.
//
//   score_text_check run ENTRIES RECORDS BUDGET FLAGS HEAP STRIDE DESCRIPTOR-ARGUMENTS...
// As score_check, for an image opened with FLAGS (1 checked, 2 text) over planes of stride 1 and a heap of HEAP bytes:
// "REFUSED <words>", or "IMAGE ..." and a line for every record,
//   A <kind> <the SCORE's double as 16 hex digits> <length> <the score column as hex digits>
//   R 0 0000000000000000 0 -
//   S 0 0000000000000000 0 - <words>
// STRIDE > 0: the rule writes the score column into a row of STRIDE bytes; 0: no row (a string SCORE stops).  The host
// side is ScoreVM::run and HitPrinter::print: the column is what print writes between the blank behind the name and
// the strand.  The two must agree: outcome, kind, bits, column; for a stop the host VM has too, its words.  A stop the
// host VM has not -- the budget, the heap, the row, a directive the VM only notes an error on, a conversion the device
// does not write, bits() beyond the table -- must meet a host VM that did not fail.  "MISMATCH record ..." and status 1
// otherwise.  "BITS <calls> <calls over a window with fewer than four distinct letters>" at the end counts the rule's
// calls of bits().
#include "rm_cli.h"
#include "rm_score.h"
static long	bits_calls = 0, bits_few = 0;
#define RMS_ON_BITS( letters, len )	( bits_calls++, bits_few += ( letters ) < 4 )
#include "rm_score_core.h"
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <thread>

using namespace rma;

namespace {

std::vector<char> slurp( const char *path )
{
	std::ifstream	f( path, std::ios::binary );
	if( !f ){
		fprintf( stderr, "score_text_check: cannot read %s\n", path );
		exit( 2 );
	}
	return std::vector<char>( std::istreambuf_iterator<char>( f ), std::istreambuf_iterator<char>() );
}

char wc_cmp( char c )		// mk_rcmp, rnamot.c:193-216
{
	switch( c ){
	case 'a' : case 'A' : return 't';
	case 'c' : case 'C' : return 'g';
	case 'g' : case 'G' : return 'c';
	case 't' : case 'T' : case 'u' : case 'U' : return 'a';
	default : return 'n';
	}
}

struct HostBases {
	const char	*s;
	int	slen;
	unsigned char	operator()( int i ) const { return unsigned( i ) < unsigned( slen ) ? static_cast<unsigned char>( s[ i ] ) : 'n'; }
};

uint64_t bits_of( double d )
{
	uint64_t	u;
	memcpy( &u, &d, sizeof( u ) );
	return u;
}

// ---------------------------------------------------------------- the formatter alone
struct CStr {
	const char	*s;
	unsigned char	operator()( int i ) const { return static_cast<unsigned char>( s[ i ] ); }
};

struct FmtCheck {
	long	checked = 0, refused = 0, bad = 0;

	// the formatter on a directive written as C writes it: 0 and the bytes, or why not
	int	mine( const char *f, double x, int iv, const char *sv, std::string *got )
	{
		const int	len = int( strlen( f ) );
		const char	conv = f[ len - 1 ];
		RmsSpec	sp;
		if( !rms_fmt_parse( CStr{ f }, 1, len - 1, &sp ) )
			return -1;
		uint8_t	buf[ 256 ];
		memset( buf, '#', sizeof( buf ) );
		RmsSink	o{ buf, 1, 0, int( sizeof( buf ) ), 0 };
		int	rc = 0;
		if( conv == 'f' )
			rc = rms_fmt_f( o, sp, x );
		else if( conv == 's' )
			rms_fmt_str( o, sp, CStr{ sv }, int( strlen( sv ) ) );
		else
			rms_fmt_int( o, sp, static_cast<unsigned char>( conv ), iv );
		got->assign( reinterpret_cast<char *>( buf ), size_t( o.n < int( sizeof( buf ) ) ? o.n : int( sizeof( buf ) ) ) );
		return rc;
	}
	void	equal( const char *f, double x, int iv, const char *sv )
	{
		char	want[ 512 ];
		const char	conv = f[ strlen( f ) - 1 ];
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wformat-nonliteral"
#pragma GCC diagnostic ignored "-Wformat-security"
		if( conv == 'f' ) snprintf( want, sizeof( want ), f, x );
		else if( conv == 's' ) snprintf( want, sizeof( want ), f, sv );
		else if( conv == 'd' || conv == 'i' ) snprintf( want, sizeof( want ), f, iv );
		else snprintf( want, sizeof( want ), f, unsigned( iv ) );
#pragma GCC diagnostic pop
		std::string	got;
		const int	rc = mine( f, x, iv, sv, &got );
		checked++;
		if( ( rc != 0 || got != want ) && bad++ < 10 )
			printf( "BAD %s of %a / %d / '%s': snprintf [%s], the formatter %d [%s]\n", f, x, iv, sv, want, rc, got.c_str() );
	}
	void	refuses( const char *f, double x )
	{
		std::string	got;
		refused++;
		if( mine( f, x, 0, "", &got ) == 0 && bad++ < 10 )
			printf( "BAD %s of %a is outside the domain and was written as [%s]\n", f, x, got.c_str() );
	}
	void	one( const char *flags, const char *width, int prec, double x )
	{
		char	f[ 64 ];
		snprintf( f, sizeof( f ), "%%%s%s.%df", flags, width, prec );
		if( std::isfinite( x ) && fabs( x ) < 9223372036854775808.0 && prec <= RMS_FMT_MAX_PREC )
			equal( f, x, 0, "" );
		else
			refuses( f, x );
	}
};

int fmt_main( uint64_t seed, long count )
{
	static const char	*flags[] = { "", "-", "+", " ", "0", "#", "-+", "0+", "- ", "#0", "+ ", "-0", "0 ", "#+" };
	static const char	*widths[] = { "", "1", "8", "12", "30" };
	static const char	*precs[] = { "", ".", ".0", ".1", ".5", ".12" };
	const int	n_flags = int( sizeof( flags ) / sizeof( flags[ 0 ] ) ), n_widths = int( sizeof( widths ) / sizeof( widths[ 0 ] ) );
	// the random values in eight slices, each with a generator of its own ( seed + slice ), on as many threads as there are
	constexpr int	SLICES = 8;
	FmtCheck	part[ SLICES ];
	auto slice = [&]( int t ){
	FmtCheck	&c = part[ t ];
	std::mt19937_64	r( seed + uint64_t( t ) );
	for( long it = t; it < count; it += SLICES ){
		const uint64_t	u = r();
		double	x;
		switch( it % 6 ){
		case 0 : memcpy( &x, &u, 8 ); break;								// any bit pattern
		case 1 : x = double( int64_t( u >> 20 ) ) / 1024.0 * ( u & 1 ? -1 : 1 ); break;			// ten binary places
		case 2 : x = ldexp( double( u >> 11 ), -int( u % 140 ) ); break;					// every scale down to 2^-139
		case 3 : x = ( int( u % 2000001 ) - 1000000 ) * 0.5 / double( 1 << ( u >> 60 ) ); break;		// exact ties
		case 4 : { const uint64_t v = u & 0x800fffffffffffffull; memcpy( &x, &v, 8 ); break; }		// subnormals
		default : x = ldexp( double( u >> 11 ), -53 ) * ( u & 1 ? 1000.0 : -1.0 ); break;			// scores
		}
		for( int p = 0; p <= 18; p++ )
			c.one( flags[ ( it + p ) % n_flags ], widths[ ( it / 3 + p ) % n_widths ], p, x );
		c.one( "", "", 19 + int( it % 3 ), x );		// (refused)
	}
	};
	{
		std::vector<std::thread>	th;
		for( int t = 0; t < SLICES; t++ )
			th.emplace_back( slice, t );
		for( std::thread &t : th )
			t.join();
	}
	FmtCheck	c;
	for( const FmtCheck &p : part ){
		c.checked += p.checked;
		c.refused += p.refused;
		c.bad += p.bad;
	}
	const double	big = 9223372036854775808.0;
	const double	special[] = { 0.0, -0.0, 0.5, 1.5, 2.5, -0.5, 0.125, 0.375, 0.0005, -0.0004, -0.0005, nextafter( big, 0.0 ), -nextafter( big, 0.0 ),
		nextafter( nextafter( big, 0.0 ), 0.0 ), big, -big, 1e19, HUGE_VAL, -HUGE_VAL, NAN, 5e-324, 2.2250738585072014e-308, 0.9995, 999.9995, 9.5, 99.5, 1e18,
		0.05, 0.15, 0.25, 0.35, 1e-19, 5e-19, 4.9999999999999999e-19 };
	for( double x : special )
		for( int p = 0; p <= 18; p++ )
			for( const char *fl : flags )
				for( const char *w : widths )
					c.one( fl, w, p, x );
	// a tie at every precision: an odd multiple of 2^-( p + 1 ) has p + 1 binary places, and ends in 5 at decimal place p + 1
	for( int p = 0; p <= 18; p++ )
		for( int k = 1; k < 64; k += 2 ){
			c.one( "", "", p, ldexp( double( k ), -( p + 1 ) ) );
			c.one( "", "", p, -ldexp( double( k ), -( p + 1 ) ) - 3.0 );
		}
	for( int k = -20000; k <= 20000; k++ ){
		const float	e = 0.01 * k;
		for( int p = 0; p <= 18; p++ )
			c.one( p == 3 ? "" : flags[ ( k + 20000 + p ) % n_flags ], p == 3 ? "8" : widths[ ( k + 20000 ) % n_widths ], p, double( e ) );
	}
	const int	ivs[] = { 0, 1, -1, 7, 8, 9, 10, 255, -255, 2147483647, -2147483647 - 1, 123456, -98765, 1000000000 };
	for( const char *cv = "diouxX"; *cv; cv++ )
		for( int iv : ivs )
			for( const char *fl : flags )
				for( const char *w : widths )
					for( const char *pr : precs ){
						char	f[ 64 ];
						snprintf( f, sizeof( f ), "%%%s%s%s%c", fl, w, pr, *cv );
						c.equal( f, 0, iv, "" );
					}
	const char	*svs[] = { "", "a", "acgu", "0123456789abcdef" };
	for( const char *sv : svs )
		for( const char *fl : flags )
			for( const char *w : widths )
				for( const char *pr : precs ){
					char	f[ 64 ];
					snprintf( f, sizeof( f ), "%%%s%s%ss", fl, w, pr );
					c.equal( f, 0, 0, sv );
				}
	// what a directive may not hold
	std::string	got;
	for( const char *f : { "%ld", "%hd", "%lf", "%Lf", "%'d", "%*d", "%1$d", "%.*f", "%zd", "%Id" } )
		if( c.mine( f, 1.0, 1, "", &got ) != -1 && c.bad++ < 10 )
			printf( "BAD %s was parsed\n", f );
	printf( "FMT checked=%ld refused=%ld bad=%ld\n", c.checked, c.refused, c.bad );
	return c.bad != 0;
}

}	// namespace

int main( int argc, char **argv )
{
	if( argc == 4 && !strcmp( argv[ 1 ], "fmt" ) )
		return fmt_main( strtoull( argv[ 2 ], nullptr, 10 ), atol( argv[ 3 ] ) );
	if( argc < 9 || strcmp( argv[ 1 ], "run" ) ){
		fprintf( stderr, "usage: score_text_check fmt SEED COUNT | run ENTRIES RECORDS BUDGET FLAGS HEAP STRIDE DESCRIPTOR-ARGUMENTS...\n" );
		return 2;
	}
	const std::vector<char>	eb = slurp( argv[ 2 ] ), rb = slurp( argv[ 3 ] );
	int	budget = atoi( argv[ 4 ] );
	if( budget <= 0 )
		budget = RMS_DEFAULT_BUDGET;
	const unsigned	flags = unsigned( atoi( argv[ 5 ] ) );
	const int	heap_cap = atoi( argv[ 6 ] ), row_cap = atoi( argv[ 7 ] );
	std::vector<char *>	av{ argv[ 0 ] };
	for( int i = 8; i < argc; i++ )
		av.push_back( argv[ i ] );
	Prepared	pr;
	try{
		pr = prepare( parse_args( int( av.size() ), av.data() ) );
	}catch( Error &e ){
		fprintf( stderr, "score_text_check: %s\n", e.what() );
		return 2;
	}
	Descriptor	&d = *pr.descr;
	const rma_program_t	&prog = *pr.prog;
	ScoreImage	img;
	const std::string	why = score_image_make_flags( d, prog, &img, flags );
	if( !why.empty() ){
		printf( "REFUSED %s\n", why.c_str() );
		return 0;
	}
	const RmsImage	*m = img.image();
	printf( "IMAGE inst=%d vars=%d deepest=%d stack=%d bytes=%d pool=%d pairsets=%d wave_bytes=%d flags=%d bits_L=%d table=%zu\n", m->n_inst, m->n_vars,
		img.deepest, m->stack, m->bytes, m->n_pool, m->n_ps, rms_wave_bytes( m->stack, m->n_vars ), m->flags, m->bits_L, img.bits_tab.size() );

	const int32_t	*ew = reinterpret_cast<const int32_t *>( eb.data() );
	const int	n_seq = eb.size() >= 4 ? ew[ 0 ] : 0;
	std::vector<const char *>	text( static_cast<size_t>( n_seq ), nullptr );
	const char	*tp = eb.data() + 4 * ( size_t( n_seq ) + 1 );
	for( int i = 0; i < n_seq; i++ ){
		text[ size_t( i ) ] = tp;
		tp += ew[ 1 + i ];
	}
	const int	stride = rma_hit_stride( &prog ), ctx_off = rma_hit_ctx_off( &prog ), efn_off = rma_hit_efn_off( &prog );
	const int64_t	n = int64_t( rb.size() / 4 / size_t( stride ) );
	const int32_t	*recs = reinterpret_cast<const int32_t *>( rb.data() );

	// Replayer::begin()
	d.score->setprog( P_BEGIN );
	d.score->run( 0, 0, nullptr, nullptr, nullptr );
	d.score->setprog( P_MAIN );
	char	*pbuf = nullptr;
	size_t	psize = 0;
	FILE	*pf = open_memstream( &pbuf, &psize );
	HitPrinter	printer( d, pf );

	std::vector<int32_t>	planes( size_t( m->stack + m->n_vars ) * 3 );
	std::vector<uint8_t>	estk( RMS_ESTK ), heap( size_t( heap_cap ) + 4 ), row( size_t( row_cap ) + 4 );
	RmsMem<1>	mem{ planes.data(), estk.data(), m->stack, m->n_vars };
	mem.heap = heap.data();
	mem.heap_cap = heap_cap;
	RmsText	tx;
	tx.bits_tab = img.bits_tab.empty() ? nullptr : img.bits_tab.data();
	if( row_cap > 0 ){
		tx.row = row.data();
		tx.row_cap = row_cap;
	}
	std::string	rc;
	int	cur = -1, status = 0;
	for( int64_t h = 0; h < n; h++ ){
		const int32_t	*w = recs + h * stride;
		const int	seq = w[ 0 ], comp = w[ 1 ];
		if( seq < 0 || seq >= n_seq || ( comp != 0 && comp != 1 ) ){
			fprintf( stderr, "score_text_check: record %lld: entry %d, strand %d\n", ( long long )h, seq, comp );
			return 2;
		}
		const int	slen = ew[ 1 + seq ];
		if( comp && seq != cur ){
			rc.assign( size_t( slen ), 'n' );
			for( int i = 0; i < slen; i++ )
				rc[ size_t( slen - 1 - i ) ] = wc_cmp( text[ size_t( seq ) ][ i ] );
			cur = seq;
		}
		std::string	fwd;
		const char	*sbuf;
		if( comp )
			sbuf = rc.c_str();
		else{
			fwd.assign( text[ size_t( seq ) ], size_t( slen ) );		// (the VM's strings end with a NUL)
			sbuf = fwd.c_str();
		}
		// ---- the host VM, the record restored as Replayer::one_hit restores it
		int	len = 0;
		for( int e = 0; e < prog.n_elems; e++ ){
			Strel	&s = d.descr[ size_t( e ) ];
			s.matchoff = w[ RMA_HIT_HDR + 4 * e ];
			s.matchlen = w[ RMA_HIT_HDR + 4 * e + 1 ];
			s.n_mispairs = w[ RMA_HIT_HDR + 4 * e + 2 ];
			s.n_mismatches = w[ RMA_HIT_HDR + 4 * e + 3 ];
			len += s.matchlen;
		}
		if( d.lctx ){
			d.lctx->matchoff = w[ ctx_off ];
			d.lctx->matchlen = w[ ctx_off + 1 ];
		}
		if( d.rctx ){
			d.rctx->matchoff = w[ ctx_off + 2 ];
			d.rctx->matchlen = w[ ctx_off + 3 ];
		}
		d.nval->pval = const_cast<char *>( "e" );
		d.cval->ival = comp;
		d.pval->ival = comp ? slen - d.descr[ 0 ].matchoff : d.descr[ 0 ].matchoff + 1;
		d.lval->ival = len;
		char	vm_out = 'R';
		int	vm_kind = 0;
		uint64_t	vm_bits = 0;
		std::string	vm_words, vm_field;
		try{
			Ident	*h_id = nullptr;
			if( d.score->run( comp, slen, sbuf, &h_id, prog.n_efn_sites ? w + efn_off : nullptr ) != SA_REJECT ){
				vm_out = 'A';
				const Value	*sv = d.sval;
				if( sv->type == T_INT ){
					vm_kind = RMS_KIND_INT;
					vm_bits = bits_of( double( sv->ival ) );
				}else if( sv->type == T_FLOAT ){
					vm_kind = RMS_KIND_FLOAT;
					vm_bits = bits_of( sv->dval );
				}else if( sv->type == T_STRING )
					vm_kind = RMS_KIND_STRING;
				// the printed line: the name in 12 columns, a blank, the score column, then what follows here
				fflush( pf );
				const size_t	from = psize;
				printer.print( "e", "", comp, slen, sbuf, nullptr );
				fflush( pf );
				std::string	out( pbuf + from, psize - from );
				out.erase( 0, out.rfind( '\n', out.size() - 2 ) + 1 );		// (the line behind the header and the definition line)
				char	tail[ 64 ];
				snprintf( tail, sizeof( tail ), " %d %7d %4d ", comp, d.pval->ival, len );
				const size_t	at = out.rfind( tail );
				if( out.size() < 13 || at == std::string::npos || at < 13 ){
					fprintf( stderr, "score_text_check: record %lld: a printed line without its columns: %s", ( long long )h, out.c_str() );
					return 2;
				}
				vm_field = out.substr( 13, at - 13 );
			}
		}catch( Error &e ){
			vm_out = 'S';
			vm_words = e.what();
		}
		// ---- the rule
		RmsResult	r;
		rms_run( m, w, slen, HostBases{ sbuf, slen }, mem, budget, &r, tx );
		const char	out = r.outcome == RMS_ACCEPT ? 'A' : r.outcome == RMS_REJECT ? 'R' : 'S';
		const std::string	words = out == 'S' ? score_stop_text( img, r ) : "";
		const uint64_t	bits = out == 'A' ? bits_of( r.score ) : 0;
		const std::string	field = out == 'A' && row_cap > 0 ? std::string( reinterpret_cast<char *>( row.data() ), size_t( r.text_len ) ) : "";
		std::string	hex = field.empty() ? "-" : "";
		for( unsigned char ch : field ){
			char	b[ 4 ];
			snprintf( b, sizeof( b ), "%02x", ch );
			hex += b;
		}
		printf( "%c %d %016" PRIx64 " %d %s%s%s\n", out, out == 'A' ? r.kind : 0, bits, out == 'A' ? r.text_len : 0, hex.c_str(), out == 'S' ? " " : "", words.c_str() );
		bool	same;
		if( out == 'S' )
			switch( r.stop ){
			case RMS_STOP_BUDGET : case RMS_STOP_STRCAT : case RMS_STOP_SCORE_STRING : case RMS_STOP_HEAP : case RMS_STOP_TEXT_ROOM : case RMS_STOP_TEXT_RANGE :
			case RMS_STOP_SPF_NO_ARG : case RMS_STOP_SPF_NEED_FLOAT : case RMS_STOP_SPF_NEED_INT : case RMS_STOP_SPF_NEED_STRING : case RMS_STOP_SPF_UNSUPPORTED :
			case RMS_STOP_SPF_EG : case RMS_STOP_SPF_MODIFIER : case RMS_STOP_SPF_PREC : case RMS_STOP_SPF_RANGE : case RMS_STOP_BITS_SPAN :
				same = vm_out != 'S';		// (the host VM has the room, or goes on behind a noted error)
				break;
			default :
				same = vm_out == 'S' && words == vm_words;
				break;
			}
		else
			same = out == vm_out && ( out != 'A' || ( r.kind == vm_kind && bits == ( vm_kind == RMS_KIND_STRING ? 0 : vm_bits ) && ( row_cap == 0 || field == vm_field ) ) );
		if( !same && status == 0 ){
			printf( "MISMATCH record %lld: the VM %c %d %016" PRIx64 " [%s] %s; the rule %c %d %016" PRIx64 " [%s] %s (pc %d)\n", ( long long )h, vm_out, vm_kind,
				vm_bits, vm_field.c_str(), vm_words.c_str(), out, r.kind, bits, field.c_str(), words.c_str(), r.pc );
			status = 1;
		}
	}
	printf( "BITS %ld %ld\n", bits_calls, bits_few );
	fclose( pf );
	free( pbuf );
	return status;
}
