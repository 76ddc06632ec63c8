// struct_energy_check.cpp -- TEST INFRASTRUCTURE.
//
// rnamotif_amd/csrc/rm_structenergy.h compiled for the CPU: the check that rma_structure_energies makes of a batch of
// structures, and efn() / efn2() of the accepted ones through the cores rm_efn_core.h / rm_efn2_core.h -- with the int16
// table image the kernel stages, without and with the cache of codes and partners, with the instance of the cores
// the helix count picks (and, where that is the usual one, with the large stacks as well: the two must agree).
// tests/test_structure_energy_cpu.py builds and runs it, once more with -fsanitize=address,undefined.
//
//   struct_energy_check EFNDATA batch FILE     a batch as the call takes it:  n total / off[ n + 1 ] / the letters
//                                              (- for none) / pair[ total ];  prints "refused S REASON WHICH" or one
//                                              line "S efn efn2 helices inf" per structure
//   struct_energy_check EFNDATA time FILE REPS the batch's energies REPS times over, one way, on this core: nanoseconds a
//                                              structure for efn() and for efn2() (profiles/structure_energy.py)
//   struct_energy_check EFNDATA cross SEED N   N random symmetric pair tables of 2 to 200 bases, with crossing pairs
//                                              wherever four bases or more allow them: each must be accepted and
//                                              flagged infinite, as a quadratic search for a crossing says it should
//   struct_energy_check EFNDATA nested SEED N  N random nested structures of 1 to 300 bases over a c g u n, any letters
//                                              paired, pairs (i, i+1) among them: each must be accepted, flagged
//                                              infinite exactly where it has such a pair, and evaluate alike four ways
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <memory>
#include <random>
#include <string>
#include <vector>
#include "rm_efndata.h"
#include "rm_structenergy.h"

static const char *const	reason[] = { "ok", "off_first", "off_decreases", "off_outside", "off_last", "too_long",
	"pair_range", "pair_self", "pair_asym", "helices" };

struct Tables {
	std::unique_ptr<rma_efndata_t>	efn{ new rma_efndata_t };
	std::unique_ptr<rma_efn2data_t>	efn2{ new rma_efn2data_t };
	std::vector<int16_t>	t16;
	std::vector<int32_t>	tlkey;
	rme_tables_t	T;
	uint8_t	code[ 256 ];
};

// the energies of a checked structure, every way the kernel can take them; false: two ways disagree
static bool energies( const Tables &t, const uint8_t *base, const int32_t *pair, int len, int info, int *e, int *e2 )
{
	if( ( info & RMSE_INFO_INF ) || len <= 0 ){
		*e = RME_INF;
		*e2 = RME2_INF;
		return true;
	}
	const bool	big = rmse_info_big( info );
	int	got[ 4 ][ 2 ], n = 0;
	for( int cached = 0; cached < 2; cached++ )
		for( int inst = 0; inst < 2; inst++ ){
			if( inst == 0 && big )
				continue;	// (the usual stacks are too small: the kernel does not run them on this one)
			rme_struct_cand_t	c{ base, { pair, 1 }, t.code, len };
			std::vector<int16_t>	bp( size_t( len ) + 1 );
			std::vector<uint8_t>	bc( size_t( len ) + 4 );
			if( cached )
				c.fill_cache( bp.data(), bc.data() );
			got[ n ][ 0 ] = inst ? rme_struct_energy<1>( &t.T, c ) : rme_struct_energy<0>( &t.T, c );
			got[ n ][ 1 ] = inst ? rme2_struct_energy<1>( t.efn2.get(), c ) : rme2_struct_energy<0>( t.efn2.get(), c );
			n++;
		}
	*e = got[ 0 ][ 0 ];
	*e2 = got[ 0 ][ 1 ];
	for( int k = 1; k < n; k++ )
		if( got[ k ][ 0 ] != *e || got[ k ][ 1 ] != *e2 )
			return false;
	return true;
}

static int batch( const Tables &t, const char *path, int time_reps )
{
	FILE	*fp = fopen( path, "r" );
	if( fp == nullptr ){
		perror( path );
		return 2;
	}
	long long	n = 0, total = 0;
	if( fscanf( fp, "%lld %lld", &n, &total ) != 2 || n < 0 || total < 0 )
		return 2;
	std::vector<long long>	off( size_t( n ) + 1 );
	for( long long &o : off )
		if( fscanf( fp, "%lld", &o ) != 1 )
			return 2;
	std::vector<char>	text( size_t( total ) + 2 );
	char	fmt[ 32 ];
	snprintf( fmt, sizeof( fmt ), "%%%llds", total + 1 );
	if( fscanf( fp, fmt, text.data() ) != 1 || ( total > 0 && ( long long )strlen( text.data() ) != total ) )
		return 2;
	std::vector<int32_t>	pair( size_t( total ) + 1 );
	for( long long i = 0; i < total; i++ )
		if( fscanf( fp, "%d", &pair[ size_t( i ) ] ) != 1 )
			return 2;
	fclose( fp );
	std::vector<int>	info( size_t( n ) + 1 );
	for( long long s = 0; s < n; s++ ){
		const long long	lo = off[ size_t( s ) ], hi = off[ size_t( s ) + 1 ];
		int	r = rmse_check_offsets( lo, hi, s, n, total ), which = 0;
		if( r == RMSE_OK )
			r = rmse_check_structure( rmse_pairs_t{ pair.data() + lo, 1 }, int( hi - lo ), &which, &info[ size_t( s ) ] );
		if( r != RMSE_OK ){
			printf( "refused %lld %s %d\n", s, reason[ r ], which );
			return 0;
		}
	}
	const uint8_t	*base = reinterpret_cast<const uint8_t *>( text.data() );
	if( time_reps > 0 ){
		// one core, one way -- the cache where the kernel would use it, the instance the helix count picks -- each energy by itself
		long long	sum = 0;
		double	ns[ 2 ];
		for( int which = 0; which < 2; which++ ){
			const auto	t0 = std::chrono::steady_clock::now();
			for( int rep = 0; rep < time_reps; rep++ )
				for( long long s = 0; s < n; s++ ){
					const long long	lo = off[ size_t( s ) ];
					const int	len = int( off[ size_t( s ) + 1 ] - lo ), w = info[ size_t( s ) ];
					if( ( w & RMSE_INFO_INF ) || len <= 0 )
						continue;
					rme_struct_cand_t	c{ base + lo, { pair.data() + lo, 1 }, t.code, len };
					int16_t	bp[ RMSE_CACHE + 1 ];
					uint8_t	bc[ RMSE_CACHE + 4 ];
					if( len <= RMSE_CACHE )
						c.fill_cache( bp, bc );
					if( which == 0 )
						sum += rmse_info_big( w ) ? rme_struct_energy<1>( &t.T, c ) : rme_struct_energy<0>( &t.T, c );
					else
						sum += rmse_info_big( w ) ? rme2_struct_energy<1>( t.efn2.get(), c ) : rme2_struct_energy<0>( t.efn2.get(), c );
				}
			ns[ which ] = std::chrono::duration<double, std::nano>( std::chrono::steady_clock::now() - t0 ).count() / ( double( n ) * time_reps );
		}
		printf( "%lld structures x %d: efn %.1f ns a structure, efn2 %.1f ns (sum %lld)\n", n, time_reps, ns[ 0 ], ns[ 1 ], sum );
		return 0;
	}
	for( long long s = 0; s < n; s++ ){
		const long long	lo = off[ size_t( s ) ];
		const int	len = int( off[ size_t( s ) + 1 ] - lo ), w = info[ size_t( s ) ];
		int	e = 0, e2 = 0;
		if( !energies( t, base + lo, pair.data() + lo, len, w, &e, &e2 ) ){
			fprintf( stderr, "structure %lld: the cache or the instance changes an energy\n", s );
			return 1;
		}
		printf( "%lld %d %d %d %d\n", s, e, e2, w & 0xff, ( w & RMSE_INFO_INF ) ? 1 : 0 );
	}
	return 0;
}

static bool crosses( const std::vector<int32_t> &p )
{
	const int	len = int( p.size() );
	for( int i = 0; i < len; i++ )
		for( int k = i + 1; p[ size_t( i ) ] > i && k < p[ size_t( i ) ]; k++ )
			if( p[ size_t( k ) ] != -1 && ( p[ size_t( k ) ] < i || p[ size_t( k ) ] > p[ size_t( i ) ] ) )
				return true;
	return false;
}

static int fuzz( const Tables &t, bool nested, unsigned seed, int count )
{
	std::mt19937	rng( seed );
	auto	upto = [&]( int n ){ return int( rng() % unsigned( n ) ); };	// [0, n)
	int	n_inf = 0, n_fin = 0;
	for( int c = 0; c < count; c++ ){
		const int	len = nested ? 1 + upto( 300 ) : 2 + upto( 199 );
		std::vector<int32_t>	p( size_t( len ), -1 );
		std::string	seq( size_t( len ), 'a' );
		for( char &ch : seq )
			ch = "acgun"[ upto( 100 ) < 3 ? 4 : upto( 4 ) ];
		bool	adjacent = false;
		if( nested ){
			// helices laid into free intervals, outermost first; at most 45 of them
			std::vector<std::pair<int, int>>	free_iv{ { 0, len - 1 } };
			for( int h = 0; h < 45 && !free_iv.empty(); h++ ){
				const size_t	at = size_t( upto( int( free_iv.size() ) ) );
				const std::pair<int, int>	iv = free_iv[ at ];
				free_iv.erase( free_iv.begin() + long( at ) );
				const int	room = iv.second - iv.first + 1;
				const bool	adj = upto( 60 ) == 0;		// a pair (i, i+1) now and then
				if( room < ( adj ? 2 : 3 ) )
					continue;
				const int	i = iv.first + upto( std::min( room - ( adj ? 1 : 2 ), 6 ) );
				const int	j = adj ? i + 1 : iv.second - upto( std::min( iv.second - i - 1, 6 ) );
				int	k = 0;
				const int	most = 1 + upto( 6 );
				while( k < most && ( j - k ) - ( i + k ) >= ( adj ? 1 : 2 ) ){
					p[ size_t( i + k ) ] = j - k;
					p[ size_t( j - k ) ] = i + k;
					adjacent |= i + k + 1 == j - k;
					k++;
				}
				if( iv.first <= i - 1 )
					free_iv.push_back( { iv.first, i - 1 } );
				if( i + k <= j - k )
					free_iv.push_back( { i + k, j - k } );
				if( j + 1 <= iv.second )
					free_iv.push_back( { j + 1, iv.second } );
			}
		}else{
			// up to 40 random pairs, tried again until two of them cross (under four bases none can: those tables are
			// merely symmetric)
			do{
				std::fill( p.begin(), p.end(), -1 );
				const int	pairs = len < 4 ? 1 : 2 + upto( std::min( len / 2, 40 ) - 1 );
				for( int k = 0; k < pairs; k++ ){
					const int	i = upto( len ), j = upto( len );
					if( i != j && p[ size_t( i ) ] == -1 && p[ size_t( j ) ] == -1 ){
						p[ size_t( i ) ] = j;
						p[ size_t( j ) ] = i;
					}
				}
			}while( len >= 4 && !crosses( p ) );
			for( int i = 0; i + 1 < len; i++ )
				adjacent |= p[ size_t( i ) ] == i + 1;
		}
		int	which = 0, info = 0;
		const int	r = rmse_check_structure( rmse_pairs_t{ p.data(), 1 }, len, &which, &info );
		const bool	want_inf = adjacent || crosses( p );
		if( r != RMSE_OK || bool( info & RMSE_INFO_INF ) != want_inf || ( nested && crosses( p ) ) ){
			fprintf( stderr, "case %d: check %s, info %#x, infinite wanted %d\n", c, reason[ r ], info, int( want_inf ) );
			return 1;
		}
		int	e = 0, e2 = 0;
		if( !energies( t, reinterpret_cast<const uint8_t *>( seq.data() ), p.data(), len, info, &e, &e2 ) ){
			fprintf( stderr, "case %d: the cache or the instance changes an energy\n", c );
			return 1;
		}
		if( want_inf && ( e != RME_INF || e2 != RME2_INF ) ){
			fprintf( stderr, "case %d: energies %d %d, not the infinities\n", c, e, e2 );
			return 1;
		}
		( want_inf ? n_inf : n_fin )++;
	}
	printf( "%d structures: %d infinite by the check, %d through the cores\n", count, n_inf, n_fin );
	return 0;
}

int main( int argc, char **argv )
{
	if( argc < 4 ){
		fprintf( stderr, "usage: struct_energy_check EFNDATA batch FILE | time FILE REPS | cross SEED N | nested SEED N\n" );
		return 2;
	}
	Tables	t;
	std::string	err;
	try{
		if( !rma::load_efndata( argv[ 1 ], t.efn.get(), err ) || !rma::load_efn2data( argv[ 1 ], t.efn2.get(), err ) ){
			fprintf( stderr, "%s\n", err.c_str() );
			return 2;
		}
	}catch( rma::Error &e ){
		fprintf( stderr, "%s\n", e.what() );
		return 2;
	}
	rma::efn_tables16( t.efn.get(), t.t16, t.tlkey );
	t.T = rme_tables_t{ t.t16.data(), t.tlkey.data(), t.efn->loginc };
	for( int b = 0; b < 256; b++ ){
		unsigned char	l = static_cast<unsigned char>( b );
		if( l >= 'A' && l <= 'Z' )
			l = static_cast<unsigned char>( l + ( 'a' - 'A' ) );
		t.code[ b ] = uint8_t( rmse_letter_code( l >= 'a' && l <= 'z' ? l : 'n' ) );
	}
	const std::string	mode = argv[ 2 ];
	if( mode == "batch" )
		return batch( t, argv[ 3 ], 0 );
	if( mode == "time" && argc >= 5 )
		return batch( t, argv[ 3 ], atoi( argv[ 4 ] ) );
	if( ( mode == "cross" || mode == "nested" ) && argc >= 5 )
		return fuzz( t, mode == "nested", unsigned( atoi( argv[ 3 ] ) ), atoi( argv[ 4 ] ) );
	fprintf( stderr, "struct_energy_check: no mode '%s'\n", mode.c_str() );
	return 2;
}
