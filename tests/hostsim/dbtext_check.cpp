// dbtext_check -- the rule of rnamotif_amd/csrc/rm_dbtext.h run on the host, the way the kernels of
// rm_dbtext_dev.hip run it, and held to PackFile::unpack.
//
//	dbtext_check pack FILE.rmdb
//		The pack's entries as four databases -- in the pack's order, in reverse order with every third entry
//		twice, without exceptions, and with every padding bit of the mask set -- each through the directory, the per-entry check and the fill, slot by
//		slot in groups of 64 as a wave takes them (a group inside one entry by the lane scan, a group over several
//		by a rank of its own per lane); every entry's text against PackFile::unpack (without exceptions: its
//		letters that are not a, c, g, t as n).  Prints "ok ENTRIES SLOTS GROUPS_ONE GROUPS_MIXED"; exit status 1
//		with the first difference otherwise.
//	dbtext_check index BASE_OFF P EXC_BASE DIR_RUN IN_RUN BELOW
//		The rule's index arithmetic: prints the code word, the mask word, its run, the run's first word, the
//		index into exc[] and the bytes of an entry of P + 1 bases, in decimal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rm_dbtext.h"
#include "rm_pack.h"

namespace {

struct Db {			// what a kernel sees: every array in a heap block of exactly its size
	std::vector<uint32_t>	codes, amask;
	std::vector<int64_t>	base_off, exc_off, text_start, exc_base;
	std::vector<int32_t>	slen;
	std::vector<char>	exc;
	std::vector<uint64_t>	dir;
	std::vector<unsigned char>	text;
	bool	has_exc = true;
	int64_t	text_bytes = 0;
};

int64_t G( const Db &d, int64_t W )
{
	int64_t	g = int64_t( d.dir[ size_t( rma::dbtext_run( W ) ) ] );
	for( int64_t i = rma::dbtext_run_first( W ); i < W; i++ )
		g += rma::dbtext_popcount( d.amask[ size_t( i ) ] );
	return g;
}

// the directory, then the per-entry check: the least bad word
unsigned long long prepare( Db &d )
{
	const int64_t	n_mask = int64_t( d.amask.size() ), runs = rma::dbtext_dir_runs( n_mask );
	d.dir.assign( size_t( runs ), 0 );
	uint64_t	sum = 0;
	for( int64_t r = 0; r < runs; r++ ){
		d.dir[ size_t( r ) ] = sum;
		for( int64_t w = r * rma::DT_RUN_WORDS; w < ( r + 1 ) * rma::DT_RUN_WORDS && w < n_mask; w++ )
			sum += uint64_t( rma::dbtext_popcount( d.amask[ size_t( w ) ] ) );
	}
	unsigned long long	bad = rma::DT_BAD_NONE;
	const size_t	n = d.slen.size();
	d.exc_base.assign( n, 0 );
	d.text_start.assign( n, 0 );
	d.text_bytes = 0;
	for( size_t e = 0; e < n; e++ ){
		d.text_start[ e ] = d.text_bytes;
		d.text_bytes += rma::dbtext_entry_bytes( d.slen[ e ] );
		const int64_t	w0 = d.base_off[ e ] / 32, w1 = w0 + ( d.slen[ e ] >> 5 );
		const int	b = d.slen[ e ] & 31;
		const int64_t	g0 = G( d, w0 );
		const int64_t	g1 = G( d, w1 ) + ( b != 0 ? rma::dbtext_popcount( d.amask[ size_t( w1 ) ] & ( ( 1u << b ) - 1u ) ) : 0 );
		if( !d.has_exc )
			continue;
		d.exc_base[ e ] = d.exc_off[ e ] - g0;
		if( g1 - g0 != d.exc_off[ e + 1 ] - d.exc_off[ e ] ){
			const unsigned long long	w = rma::dbtext_bad_word( int32_t( e ), rma::DT_BAD_COUNT, uint32_t( g1 - g0 ) );
			bad = w < bad ? w : bad;
		}
	}
	if( d.has_exc )
		for( size_t k = 0; k < d.exc.size(); k++ )
			if( !rma::dbtext_exc_letter( static_cast<unsigned char>( d.exc[ k ] ) ) ){
				const int32_t	e = rma::dbtext_entry_at( d.exc_off.data(), 0, int32_t( n ), int64_t( k ) ) - 1;
				const unsigned long long	w = rma::dbtext_bad_word( e, rma::DT_BAD_LETTER, static_cast<unsigned char>( d.exc[ k ] ) );
				bad = w < bad ? w : bad;
			}
	return bad;
}

// the fill, a group of 64 slots at a time
void fill( Db &d, int64_t *groups_one, int64_t *groups_mixed )
{
	d.text.assign( size_t( d.text_bytes ), '?' );
	const int64_t	slots = d.text_bytes / rma::DT_SLOT;
	const int32_t	n = int32_t( d.slen.size() );
	const char	*exc = d.has_exc ? d.exc.data() : nullptr;
	const int64_t	n_exc = int64_t( d.exc.size() );
	for( int64_t t0 = 0; t0 < slots; t0 += 64 ){
		const int64_t	tl = t0 + 63 < slots ? t0 + 63 : slots - 1;
		const int32_t	e0 = rma::dbtext_entry_at( d.text_start.data(), 0, n, rma::DT_SLOT * t0 ) - 1;
		const int32_t	e1 = rma::dbtext_entry_at( d.text_start.data(), e0, n, rma::DT_SLOT * tl ) - 1;
		const bool	one = e0 == e1;
		( one ? *groups_one : *groups_mixed )++;
		int	scan = 0;		// the masked bases of the lanes before
		int64_t	g0 = 0;
		int	below0 = 0;
		for( int64_t t = t0; t <= tl; t++ ){
			const int32_t	e = one ? e0 : rma::dbtext_entry_at( d.text_start.data(), e0, e1 + 1, rma::DT_SLOT * t ) - 1;
			const int64_t	cw = t - d.text_start[ size_t( e ) ] / rma::DT_SLOT;
			const int64_t	W = d.base_off[ size_t( e ) ] / 32 + ( cw >> 1 );
			const uint32_t	code = d.codes[ size_t( rma::dbtext_code_word( d.base_off[ size_t( e ) ], int32_t( 16 * cw ) ) ) ];
			const uint32_t	mw = d.amask[ size_t( rma::dbtext_mask_word( d.base_off[ size_t( e ) ], int32_t( 16 * cw ) ) ) ];
			const uint32_t	m = rma::dbtext_slot_mask( mw, cw, d.slen[ size_t( e ) ] );
			const int	below = rma::dbtext_popcount( rma::dbtext_below_slot( mw, cw ) );
			uint64_t	out[ 2 ];
			rma::dbtext_slot_plain( code, m, rma::dbtext_slot_tail( cw, d.slen[ size_t( e ) ] ), out );
			if( t == t0 ){
				g0 = G( d, W );
				below0 = below;
			}
			if( exc != nullptr && m != 0u ){
				const int64_t	idx = one ? rma::dbtext_exc_index( d.exc_base[ size_t( e ) ], g0, scan, below0 ) :
					rma::dbtext_exc_index( d.exc_base[ size_t( e ) ], G( d, W ), 0, below );
				rma::dbtext_slot_patch( m, exc, idx, n_exc, out );
			}
			scan += rma::dbtext_popcount( m );
			memcpy( d.text.data() + rma::DT_SLOT * t, out, 16 );
		}
	}
}

int fail( const char *what, long long a, long long b )
{
	printf( "FAIL %s %lld %lld\n", what, a, b );
	return 1;
}

// entries `order` of the pack as a database whose words are the pack's own
int check( const rma::PackFile &pf, const std::vector<int> &order, bool has_exc, bool dirty, int64_t *slots, int64_t *one, int64_t *mixed )
{
	Db	d;
	d.has_exc = has_exc;
	d.codes.assign( pf.codes.begin(), pf.codes.end() );
	d.amask.assign( pf.amask.begin(), pf.amask.end() );
	d.exc_off.push_back( 0 );
	for( int e : order ){
		d.base_off.push_back( pf.base_off[ size_t( e ) ] );
		d.slen.push_back( pf.slen[ size_t( e ) ] );
		const int64_t	x0 = pf.exc_off[ size_t( e ) ], x1 = e + 1 < pf.count() ? pf.exc_off[ size_t( e ) + 1 ] : int64_t( pf.exc.size() );
		d.exc.insert( d.exc.end(), pf.exc.begin() + x0, pf.exc.begin() + x1 );
		d.exc_off.push_back( int64_t( d.exc.size() ) );
	}
	if( dirty )		// padding bits set: they are never counted for a base of the entry
		for( size_t i = 0; i < d.slen.size(); i++ )
			if( d.slen[ i ] % 32 != 0 )
				d.amask[ size_t( d.base_off[ i ] / 32 + d.slen[ i ] / 32 ) ] |= ~0u << ( d.slen[ i ] % 32 );
	const unsigned long long	bad = prepare( d );
	if( bad != rma::DT_BAD_NONE )
		return fail( "check word", rma::dbtext_bad_entry( bad ), rma::dbtext_bad_value( bad ) );
	fill( d, one, mixed );
	*slots += d.text_bytes / rma::DT_SLOT;
	for( size_t i = 0; i < order.size(); i++ ){
		std::string	want = pf.unpack( order[ i ] );
		if( !has_exc )
			for( char &c : want )
				if( c != 'a' && c != 'c' && c != 'g' && c != 't' )
					c = 'n';
		const unsigned char	*got = d.text.data() + d.text_start[ i ];
		if( d.text_start[ i ] % 16 != 0 )
			return fail( "text_start", ( long long )i, ( long long )d.text_start[ i ] );
		for( size_t p = 0; p < want.size(); p++ )
			if( got[ p ] != static_cast<unsigned char>( want[ p ] ) )
				return fail( "letter", ( long long )i, ( long long )p );
		for( int64_t p = int64_t( want.size() ); p < rma::dbtext_entry_bytes( int32_t( want.size() ) ); p++ )
			if( got[ p ] != 'n' )
				return fail( "tail", ( long long )i, ( long long )p );
	}
	// the check sees what it is there for: an exception too few, one too many, a byte that is no such letter
	if( has_exc && !d.exc.empty() ){
		size_t	e = 0;
		while( d.exc_off[ e + 1 ] == d.exc_off[ e ] )
			e++;
		Db	f = d;
		for( size_t k = e + 1; k < f.exc_off.size(); k++ )
			f.exc_off[ k ]--;
		f.exc.erase( f.exc.begin() + f.exc_off[ e ] );
		unsigned long long	w = prepare( f );
		if( w == rma::DT_BAD_NONE || rma::dbtext_bad_entry( w ) != int32_t( e ) || rma::dbtext_bad_kind( w ) != rma::DT_BAD_COUNT ||
			int64_t( rma::dbtext_bad_value( w ) ) != d.exc_off[ e + 1 ] - d.exc_off[ e ] )
			return fail( "one exception too few", ( long long )e, ( long long )w );
		f = d;
		f.exc[ size_t( f.exc_off[ e ] ) ] = 'N';
		w = prepare( f );
		if( rma::dbtext_bad_entry( w ) != int32_t( e ) || rma::dbtext_bad_kind( w ) != rma::DT_BAD_LETTER || rma::dbtext_bad_value( w ) != 'N' )
			return fail( "a byte that is no letter of a masked position", ( long long )e, ( long long )w );
	}
	return 0;
}

}	// namespace

int main( int argc, char **argv )
{
	if( argc == 8 && !strcmp( argv[ 1 ], "index" ) ){
		const int64_t	base_off = strtoll( argv[ 2 ], nullptr, 10 );
		const int32_t	p = int32_t( strtoll( argv[ 3 ], nullptr, 10 ) );
		const int64_t	exc_base = strtoll( argv[ 4 ], nullptr, 10 ), dir_run = strtoll( argv[ 5 ], nullptr, 10 );
		const int64_t	in_run = strtoll( argv[ 6 ], nullptr, 10 );
		const int	below = atoi( argv[ 7 ] );
		const int64_t	mw = rma::dbtext_mask_word( base_off, p );
		printf( "%lld %lld %lld %lld %lld %lld\n", ( long long )rma::dbtext_code_word( base_off, p ), ( long long )mw,
			( long long )rma::dbtext_run( mw ), ( long long )rma::dbtext_run_first( mw ),
			( long long )rma::dbtext_exc_index( exc_base, dir_run, in_run, below ), ( long long )rma::dbtext_entry_bytes( p ) );
		return 0;
	}
	if( argc != 3 || strcmp( argv[ 1 ], "pack" ) ){
		fprintf( stderr, "usage: dbtext_check pack FILE.rmdb | index BASE_OFF P EXC_BASE DIR_RUN IN_RUN BELOW\n" );
		return 2;
	}
	rma::PackFile	pf;
	std::string	err;
	if( !pf.load( argv[ 2 ], err ) ){
		fprintf( stderr, "%s\n", err.c_str() );
		return 2;
	}
	std::vector<int>	fwd, rev;
	for( int i = 0; i < pf.count(); i++ )
		fwd.push_back( i );
	for( int i = pf.count() - 1; i >= 0; i-- ){
		rev.push_back( i );
		if( i % 3 == 0 )
			rev.push_back( i );
	}
	int64_t	slots = 0, one = 0, mixed = 0;
	if( check( pf, fwd, true, false, &slots, &one, &mixed ) || check( pf, rev, true, false, &slots, &one, &mixed ) ||
		check( pf, fwd, false, false, &slots, &one, &mixed ) || check( pf, fwd, true, true, &slots, &one, &mixed ) )
		return 1;
	printf( "ok %zu %lld %lld %lld\n", 3 * fwd.size() + rev.size(), ( long long )slots, ( long long )one, ( long long )mixed );
	return 0;
}
