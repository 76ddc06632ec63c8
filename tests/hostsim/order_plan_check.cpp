// order_plan_check.cpp -- TEST INFRASTRUCTURE.
//
// What the end of a scan depends on in a descriptor's device program (rnamotif_amd/csrc/rm_dev_program.cpp), for
// tests/scan_end_cases.py: one line
//   lean_ok L ord_ok O ord_bits B w_winsize W hit_stride S n_efn N efn_big G
// then per search level one line
//   level K elem E ord_stride T ord_nlen N
// Reads no GPU state.
//
//   order_plan_check [rnamotif options] -descr file
#include <cstdio>
#include <exception>
#include "rm_cli.h"
#include "rm_dev_program.h"

int main( int argc, char **argv )
{
	try{
		rma::Prepared	pr = rma::prepare( rma::parse_args( argc, argv ) );
		rmd_program_t	dp;
		char	err[ 512 ];
		if( rmd_build( pr.prog.get(), &dp, err, sizeof( err ) ) ){
			fprintf( stderr, "rmd_build: %s\n", err );
			return 2;
		}
		printf( "lean_ok %d ord_ok %d ord_bits %d w_winsize %d hit_stride %d n_efn %d efn_big %d\n", int( dp.lean_ok ), int( dp.ord_ok ),
			int( dp.ord_bits ), int( dp.w_winsize ), int( dp.hit_stride ), int( dp.n_efn ), int( dp.efn_big ) );
		for( int k = 0; k < dp.n_searches; k++ ){
			const rmd_elem_t	&e = dp.elems[ dp.searches[ k ] ];
			printf( "level %d elem %d ord_stride %d ord_nlen %d\n", k, int( dp.searches[ k ] ), int( e.ord_stride ), int( e.ord_nlen ) );
		}
		return 0;
	}catch( const std::exception &e ){
		fputs( e.what(), stderr );
		return 1;
	}
}
