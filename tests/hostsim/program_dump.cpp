// program_dump.cpp -- TEST INFRASTRUCTURE.
//
// The product's host front end writing what it compiled a descriptor to, for oracle/ref_find_motif_drv.c
// (the reference's matcher behind a driver of this repository's own): the bytes of the rma_program_t, then
// per element that has a seq= the string as the parser leaves it (Strel::seq, after str2seq's IUPAC
// expansion; the C ABI does not expose it) -- int32 element (-1 lctx, -2 rctx), int32 length, the bytes --
// closed by element -3.
//
//   program_dump out-file [rnamotif options] -descr file
#include <cstdio>
#include <cstring>
#include <exception>
#include "rm_cli.h"

static void put_seq( FILE *fp, int32_t which, const rma::Strel *stp )
{
	if( stp == nullptr || stp->seq == nullptr )
		return;
	const int32_t	hdr[ 2 ] = { which, int32_t( strlen( stp->seq ) ) };
	fwrite( hdr, sizeof( hdr ), 1, fp );
	fwrite( stp->seq, 1, size_t( hdr[ 1 ] ), fp );
}

int main( int argc, char **argv )
{
	if( argc < 3 ){
		fprintf( stderr, "usage: program_dump out-file [rnamotif options] -descr file\n" );
		return 2;
	}
	try{
		rma::Args	args = rma::parse_args( argc - 1, argv + 1 );
		rma::Prepared	pr = rma::prepare( args );
		FILE	*fp = fopen( argv[ 1 ], "wb" );
		if( fp == nullptr ){
			fprintf( stderr, "program_dump: can't write %s\n", argv[ 1 ] );
			return 2;
		}
		fwrite( pr.prog.get(), sizeof( rma_program_t ), 1, fp );
		const rma::Descriptor	&d = *pr.descr;
		for( size_t i = 0; i < d.descr.size(); i++ )
			put_seq( fp, int32_t( i ), &d.descr[ i ] );
		put_seq( fp, -1, d.lctx );
		put_seq( fp, -2, d.rctx );
		const int32_t	end[ 2 ] = { -3, 0 };
		fwrite( end, sizeof( end ), 1, fp );
		return fclose( fp ) == 0 ? 0 : 2;
	}catch( const std::exception &e ){
		fputs( e.what(), stderr );
		return 1;
	}
}
