// beside_plan_check.cpp -- TEST INFRASTRUCTURE.
//
// The launch shapes of rnamotif_amd/csrc/rm_launch_plan.cpp under option beside, for one descriptor over the cases of
// launch_plan_check (same CASES file, same arguments): per case three lines, "ID solo ...", "ID b0 ..." and "ID b1 ...",
// the plan with the case's own options (beside at its default), with beside = 0 and with beside = 1, every field of the
// layout key and of the plan (tests/test_beside_plan_cpu.py holds them to the rules).
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
		const std::vector<int32_t>	&slen = ints( lpath );
		rma::DbShape	db;
		db.n_seq = int32_t( slen.size() );
		// (the tiles are counted as make_tiling counts them: no slices here but the ranges' own)
		std::vector<int32_t>	lo, hi;
		if( strcmp( rpath, "-" ) != 0 )
			for( size_t i = 0; i < ints( rpath ).size(); i += 2 ){
				lo.push_back( ints( rpath )[ i ] );
				hi.push_back( ints( rpath )[ i + 1 ] );
			}
		std::vector<int64_t>	base_off;
		for( int32_t l : slen ){
			base_off.push_back( db.padded_bases );
			db.padded_bases += ( int64_t( l ) + 31 ) / 32 * 32;
			db.sum_slen += l;
		}
		db.ranges = !lo.empty();
		db.ascending = asc != 0;
		const int	which[ 3 ] = { -2, 0, 1 };		// -2: the case's options as they are
		const char	*tag[ 3 ] = { "solo", "b0", "b1" };
		for( int w = 0; w < 3; w++ ){
			rma::Options	ow = o;
			if( which[ w ] != -2 && !ow.set( "beside", which[ w ] ) ){
				fprintf( stderr, "no option beside\n" );
				return 2;
			}
			const int	spill_cap = ow.spill >= 0 ? ow.spill : SPILL_ITEMS / rma::wgs_per_wave( dp );
			const rma::ProgramPlan	pp = rma::plan_program( *pr.prog, dp, prog_bytes, spill_cap, ow );
			const rma::LayoutKey	k = rma::choose_layout( pp, ow, db, cus );
			rma::Tiling	t;
			rma::make_tiling( k, slen, base_off, lo, hi, db.padded_bases, &t );
			rma::LaunchPlan	p;
			if( rma::plan_launch( k, t.n_tiles, pp, ow, cus, &p, err, sizeof( err ) ) ){
				printf( "%s %s ERR\n", id, tag[ w ] );
				continue;
			}
			printf( "%s %s tile_t=%d dminlen=%d strands=%d group=%d qcap=%d concat=%d flush=%d n_tiles=%lld lean=%d grouped=%d pooled=%d "
				"inst=%d grid=%d tile_bytes=%d lds=%zu nib=%d drain_lds=%zu drain_grid=%d listed=%d nothing=%d light=%d beside=%d cus=%d\n",
				id, tag[ w ], k.tile_t, k.dminlen, k.strands, k.group, k.qcap, int( k.concat ), int( k.flush ), ( long long )t.n_tiles,
				int( p.lean ), int( p.grouped ), int( p.pooled ), p.inst, p.grid, p.tile_bytes, p.lds, p.drain_nib, p.drain_lds, p.drain_grid,
				int( p.listed ), int( p.walks_nothing ), int( p.efn_light ), int( p.beside ), cus );
		}
	}
	return 0;
}
