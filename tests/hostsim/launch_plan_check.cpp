// launch_plan_check.cpp -- TEST INFRASTRUCTURE.
//
// The launch shapes rm_scanner.cpp would choose (rnamotif_amd/csrc/rm_launch_plan.cpp) for one descriptor over
// databases given by their entry lengths, on a device of 256 CUs, one line per case (tests/test_launch_plan.py).
//
//   launch_plan_check CASES [rnamotif options] -descr file.descr
// CASES: lines "ID LENGTHS RANGES|- ASCENDING OPTIONS|-"; LENGTHS and RANGES files of int32 (ranges: lo, hi per
// entry); OPTIONS: name=value,... as rma_scanner_set_option() takes them, and tile / qcap as RNAMOTIF_TILE / _QCAP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "rm_cli.h"
#include "rm_launch_plan.h"

static std::vector<int32_t> read_ints( const std::string &path )
{
	std::vector<int32_t>	v;
	FILE	*fp = fopen( path.c_str(), "rb" );
	if( fp == nullptr ){
		perror( path.c_str() );
		exit( 2 );
	}
	int32_t	buf[ 4096 ];
	size_t	n;
	while( ( n = fread( buf, 4, 4096, fp ) ) > 0 )
		v.insert( v.end(), buf, buf + n );
	fclose( fp );
	return v;
}

int main( int argc, char **argv )
{
	const int	cus = 256;
	std::vector<char *>	args{ argv[ 0 ] };
	for( int i = 2; i < argc; i++ )
		args.push_back( argv[ i ] );
	rma::Prepared	pr = rma::prepare( rma::parse_args( int( args.size() ), args.data() ) );
	rmd_program_t	dp;
	char	err[ 512 ];
	if( rmd_build( pr.prog.get(), &dp, err, sizeof( err ) ) ){
		fprintf( stderr, "rmd_build: %s\n", err );
		return 2;
	}
	std::vector<char>	img( sizeof( rmd_program_t ) );
	const int	prog_bytes = int( rmd_make_image( &dp, img.data() ) );
	std::map<std::string, std::vector<int32_t>>	files;
	auto ints = [ & ]( const std::string &path ) -> const std::vector<int32_t> & {
		if( !files.count( path ) )
			files[ path ] = read_ints( path );
		return files[ path ];
	};
	FILE	*cf = fopen( argv[ 1 ], "r" );
	char	id[ 256 ], lpath[ 1024 ], rpath[ 1024 ], opts[ 1024 ];
	int	asc;
	while( cf != nullptr && fscanf( cf, "%255s %1023s %1023s %d %1023s", id, lpath, rpath, &asc, opts ) == 5 ){
		rma::Options	o;
		for( char *tok = strtok( opts, "," ); tok != nullptr && strcmp( tok, "-" ) != 0; tok = strtok( nullptr, "," ) ){
			char	*eq = strchr( tok, '=' );
			*eq = '\0';
			const int	v = atoi( eq + 1 );
			if( !strcmp( tok, "tile" ) )
				o.tile = v < 0 || v > 16384 ? 0 : v;
			else if( !strcmp( tok, "qcap" ) )
				o.qcap = v;
			else if( !o.set( tok, v ) ){
				fprintf( stderr, "no option %s\n", tok );
				return 2;
			}
		}
		// the database as the packers lay it out: every entry on a 32-base boundary, one after the other
		const std::vector<int32_t>	&slen = ints( lpath );
		std::vector<int32_t>	lo, hi;
		if( strcmp( rpath, "-" ) != 0 )
			for( size_t i = 0; i < ints( rpath ).size(); i += 2 ){
				lo.push_back( ints( rpath )[ i ] );
				hi.push_back( ints( rpath )[ i + 1 ] );
			}
		std::vector<int64_t>	base_off;
		rma::DbShape	db;
		db.n_seq = int32_t( slen.size() );
		for( int32_t l : slen ){
			base_off.push_back( db.padded_bases );
			db.padded_bases += ( int64_t( l ) + 31 ) / 32 * 32;
			db.sum_slen += l;
		}
		db.ranges = !lo.empty();
		db.ascending = asc != 0;
		const int	spill_cap = o.spill >= 0 ? o.spill : SPILL_ITEMS / rma::wgs_per_wave( dp );
		const rma::ProgramPlan	pp = rma::plan_program( *pr.prog, dp, prog_bytes, spill_cap, o );
		const rma::LayoutKey	k = rma::choose_layout( pp, o, db, cus );
		rma::Tiling	t;
		rma::make_tiling( k, slen, base_off, lo, hi, db.padded_bases, &t );
		rma::LaunchPlan	p;
		if( rma::plan_launch( k, t.n_tiles, pp, o, cus, &p, err, sizeof( err ) ) ){
			printf( "%s ERR %s\n", id, err );
			continue;
		}
		uint64_t	h = 1469598103934665603ull;		// FNV-1a over the three arrays' bytes
		auto fnv = [ & ]( const void *q, size_t nb ){
			const unsigned char	*c = static_cast<const unsigned char *>( q );
			for( size_t i = 0; i < nb; i++ ){
				h ^= c[ i ];
				h *= 1099511628211ull;
			}
		};
		fnv( t.h_tile_start.data(), t.h_tile_start.size() * 8 );
		fnv( t.h_tile_seq.data(), t.h_tile_seq.size() * 4 );
		fnv( t.h_tile_meta.data(), t.h_tile_meta.size() * 4 );
		printf( "%s tile_t=%d dminlen=%d strands=%d group=%d qcap=%d concat=%d flush=%d n_tiles=%lld hash=%016llx lean=%d grouped=%d pooled=%d "
			"inst=%d grid=%d tile_bytes=%d lds=%zu nib=%d drain_lds=%zu drain_grid=%d listed=%d nothing=%d light=%d cus=%d",
			id, k.tile_t, k.dminlen, k.strands, k.group, k.qcap, int( k.concat ), int( k.flush ), ( long long )t.n_tiles, ( unsigned long long )h,
			int( p.lean ), int( p.grouped ), int( p.pooled ), p.inst, p.grid, p.tile_bytes, p.lds, p.drain_nib, p.drain_lds, p.drain_grid,
			int( p.listed ), int( p.walks_nothing ), int( p.efn_light ), cus );
		// the first and last tile's line, and the first that spans entries
		const std::vector<int32_t>	&m = t.h_tile_meta;
		auto line = [ & ]( const char *tag, int64_t i ){
			printf( " %s=%lld:", tag, ( long long )i );
			for( int w = 0; w < RMK_META_WORDS; w++ )
				printf( "%s%d", w ? "," : "", m[ size_t( i ) * RMK_META_WORDS + w ] );
		};
		if( !m.empty() && t.n_tiles > 0 ){
			line( "m0", 0 );
			line( "mN", t.n_tiles - 1 );
			for( int64_t i = 0; k.concat && i < t.n_tiles; i++ )
				if( m[ size_t( i ) * RMK_META_WORDS + RMK_META_PAD ] > 1 ){
					line( "span", i );
					break;
				}
		}
		printf( "\n" );
	}
	return 0;
}
