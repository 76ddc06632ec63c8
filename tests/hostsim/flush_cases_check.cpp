// flush_cases_check.cpp -- TEST INFRASTRUCTURE.
//
// What a descriptor's device program holds of the look-ahead chain (rmd_chain_t, rm_dev_program.cpp) and which
// search instance rm_scanner.cpp would launch for it (rm_launch_plan.cpp) over databases given by their entry
// lengths, on a device of 256 CUs: tests/test_flush_vectors_cases.py checks with it, on the CPU, that the cases of
// tests/test_flush_vectors_gpu.py run the code they are there for.
//
//   flush_cases_check CASES [rnamotif options] -descr file.descr
// CASES: lines "ID LENGTHS OPTIONS|-"; LENGTHS: a file of int32; OPTIONS: name=value,... as rma_scanner_set_option()
// takes them, and tile as RNAMOTIF_TILE.  Prints one line "chain ...", one "sib ..." per group of the chain and one
// "case ID ..." per case.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rm_cli.h"
#include "rm_launch_plan.h"

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
	const rmd_chain_t	&ch = dp.chain;
	printf( "chain on=%d n=%d s_lo=%d s_hi=%d hn_on=%d\n", int( ch.on ), int( ch.n ), int( ch.s_lo ), int( ch.s_hi ), int( ch.hn_on ) );
	for( int k = 0; k < ch.n; k++ ){
		const rmd_chain_sib_t	&sb = ch.sib[ k ];
		printf( "sib leaf=%d hmin=%d tmax=%d lmin=%d lmax=%d len_lo=%d len_hi=%d core_slot=%d\n", int( sb.leaf ), int( sb.hmin ), int( sb.tmax ),
			int( sb.lmin ), int( sb.lmax ), int( sb.len_lo ), int( sb.len_hi ), int( sb.core_slot ) );
	}
	FILE	*cf = fopen( argv[ 1 ], "r" );
	char	id[ 256 ], lpath[ 1024 ], opts[ 1024 ];
	while( cf != nullptr && fscanf( cf, "%255s %1023s %1023s", id, lpath, opts ) == 3 ){
		rma::Options	o;
		for( char *tok = strtok( opts, "," ); tok != nullptr && strcmp( tok, "-" ) != 0; tok = strtok( nullptr, "," ) ){
			char	*eq = strchr( tok, '=' );
			*eq = '\0';
			const int	v = atoi( eq + 1 );
			if( !strcmp( tok, "tile" ) )
				o.tile = v < 0 || v > 16384 ? 0 : v;
			else if( !o.set( tok, v ) ){
				fprintf( stderr, "no option %s\n", tok );
				return 2;
			}
		}
		std::vector<int32_t>	slen;
		FILE	*fp = fopen( lpath, "rb" );
		int32_t	one;
		while( fp != nullptr && fread( &one, 4, 1, fp ) == 1 )
			slen.push_back( one );
		if( fp != nullptr )
			fclose( fp );
		// the database as the packers lay it out: every entry on a 32-base boundary, one after the other
		std::vector<int32_t>	lo, hi;
		std::vector<int64_t>	base_off;
		rma::DbShape	db;
		db.n_seq = int32_t( slen.size() );
		for( int32_t l : slen ){
			base_off.push_back( db.padded_bases );
			db.padded_bases += ( int64_t( l ) + 31 ) / 32 * 32;
			db.sum_slen += l;
		}
		db.ranges = false;
		db.ascending = true;
		const int	spill_cap = o.spill >= 0 ? o.spill : SPILL_ITEMS / rma::wgs_per_wave( dp );
		const rma::ProgramPlan	pp = rma::plan_program( *pr.prog, dp, prog_bytes, spill_cap, o );
		const rma::LayoutKey	k = rma::choose_layout( pp, o, db, cus );
		rma::Tiling	t;
		rma::make_tiling( k, slen, base_off, lo, hi, db.padded_bases, &t );
		rma::LaunchPlan	p;
		if( rma::plan_launch( k, t.n_tiles, pp, o, cus, &p, err, sizeof( err ) ) ){
			printf( "case %s ERR %s\n", id, err );
			continue;
		}
		printf( "case %s tile_t=%d n_tiles=%lld inst=%s grouped=%d concat=%d nothing=%d\n", id, k.tile_t, ( long long )t.n_tiles,
			p.inst == RMK_LEAN_FLUSH ? "lean_flush" : p.inst == RMK_LEAN_CONCAT_FLUSH ? "lean_concat_flush" : p.inst == RMK_LEAN_GROUP ? "lean_group" : "other",
			int( p.grouped ), int( k.concat ), int( p.walks_nothing ) );
	}
	return 0;
}
