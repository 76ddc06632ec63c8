// hit_structures_check.cpp -- TEST INFRASTRUCTURE.
//
// The rule of rnamotif_amd/csrc/rm_hitstruct.h (what the fill kernel of rm_hitstruct_dev.hip writes per base of a hit
// record's window) run on the CPU, for tests/test_hit_structures_cpu.py and as the expected answer of
// tests/test_hit_structures.py:
//
//   hit_structures_check fill PROGRAM ENTRIES RECORDS OUT
//     PROGRAM: the rma_program_t blob of a compiled descriptor; ENTRIES: int32 n, int32 slen[ n ], then the entries'
//     raw bytes one after the other; RECORDS: int32 records of the program's stride.  Writes OUT: int64 n_records,
//     int64 off[ n + 1 ], int32 lo[ n ], uint8 base[ T ], int16 elem[ T ], int32 mate[ T ][ 3 ].  Exit status 1 and
//     "record H is bad" for a record hitstruct_check refuses.
//   hit_structures_check check PROGRAM ENTRIES RECORDS -
//     one line per record: "code which" of rma::hitstruct_check (ENTRIES may declare lengths only).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rm_hitstruct.h"

static std::vector<char> read_file( const char *path )
{
	std::vector<char>	v;
	FILE	*fp = fopen( path, "rb" );
	if( fp == nullptr ){
		perror( path );
		exit( 2 );
	}
	char	buf[ 65536 ];
	size_t	n;
	while( ( n = fread( buf, 1, sizeof( buf ), fp ) ) > 0 )
		v.insert( v.end(), buf, buf + n );
	fclose( fp );
	return v;
}

template<class T> static void put( FILE *fp, const std::vector<T> &v )
{
	if( !v.empty() && fwrite( v.data(), sizeof( T ), v.size(), fp ) != v.size() ){
		perror( "write" );
		exit( 2 );
	}
}

int main( int argc, char **argv )
{
	if( argc != 6 ){
		fprintf( stderr, "usage: %s fill|check PROGRAM ENTRIES RECORDS OUT|-\n", argv[ 0 ] );
		return 2;
	}
	const std::string	mode = argv[ 1 ];
	const std::vector<char>	blob = read_file( argv[ 2 ] );
	if( blob.size() != sizeof( rma_program_t ) ){
		fprintf( stderr, "%s: %zu bytes, a program has %zu\n", argv[ 2 ], blob.size(), sizeof( rma_program_t ) );
		return 2;
	}
	std::vector<rma_program_t>	progs( 1 );
	memcpy( progs.data(), blob.data(), sizeof( rma_program_t ) );
	const rma_program_t	&prog = progs[ 0 ];
	if( prog.magic != RMA_MAGIC || prog.size != sizeof( rma_program_t ) ){
		fprintf( stderr, "%s: not a program\n", argv[ 2 ] );
		return 2;
	}
	const std::vector<char>	ent = read_file( argv[ 3 ] );
	int32_t	n = 0;
	memcpy( &n, ent.data(), 4 );
	std::vector<int32_t>	slen( static_cast<size_t>( n ) );
	memcpy( slen.data(), ent.data() + 4, size_t( n ) * 4 );
	const std::vector<char>	rec_bytes = read_file( argv[ 4 ] );
	std::vector<int32_t>	recs( rec_bytes.size() / 4 );
	memcpy( recs.data(), rec_bytes.data(), recs.size() * 4 );
	const int	stride = rma_hit_stride( &prog );
	const int64_t	n_rec = int64_t( recs.size() ) / stride;
	const rma::HitWinShape	shape = rma::hitwin_shape( prog );
	const rma::HitStructTable	tab = rma::hitstruct_table( prog );

	if( mode == "check" ){
		for( int64_t h = 0; h < n_rec; h++ ){
			int32_t	lo, hi;
			int	which;
			const int	r = rma::hitstruct_check( recs.data() + h * stride, tab, shape, n, slen.data(), &lo, &hi, &which );
			printf( "%d %d\n", r, which );
		}
		return 0;
	}
	std::vector<size_t>	at( static_cast<size_t>( n ) );
	size_t	a = 4 + size_t( n ) * 4;
	for( int i = 0; i < n; i++ ){
		at[ i ] = a;
		a += size_t( slen[ i ] );
	}
	if( a > ent.size() ){
		fprintf( stderr, "%s: the entries' bytes end before the last entry does\n", argv[ 3 ] );
		return 2;
	}
	std::vector<int64_t>	off{ 0 };
	std::vector<int32_t>	lo_of, mate;
	std::vector<uint8_t>	base;
	std::vector<int16_t>	elem;
	for( int64_t h = 0; h < n_rec; h++ ){
		const int32_t	*w = recs.data() + h * stride;
		int32_t	lo, hi;
		int	which;
		if( rma::hitstruct_check( w, tab, shape, n, slen.data(), &lo, &hi, &which ) != rma::HW_OK ){
			fprintf( stderr, "record %lld is bad\n", ( long long )h );
			return 1;
		}
		const int	e = w[ 0 ], comp = w[ 1 ];
		const int64_t	m = rma::hitwin_len( lo, hi );
		for( int64_t i = 0; i < m; i++ ){
			const unsigned char	l = rma::hitwin_reader_letter( static_cast<unsigned char>( ent[ at[ e ] + size_t( rma::hitwin_src( comp, slen[ e ], lo, i ) ) ] ) );
			base.push_back( comp ? rma::hitwin_wc_cmp( l ) : l );
			int	el;
			int32_t	mt[ 3 ];
			rma::hitstruct_base( w, tab, shape, lo, i, &el, mt );
			elem.push_back( int16_t( el ) );
			mate.insert( mate.end(), mt, mt + 3 );
		}
		off.push_back( int64_t( base.size() ) );
		lo_of.push_back( lo );
	}
	FILE	*fp = fopen( argv[ 5 ], "wb" );
	if( fp == nullptr ){
		perror( argv[ 5 ] );
		return 2;
	}
	put( fp, std::vector<int64_t>{ n_rec } );
	put( fp, off );
	put( fp, lo_of );
	put( fp, base );
	put( fp, elem );
	put( fp, mate );
	fclose( fp );
	return 0;
}
