// hit_align_check.cpp -- TEST INFRASTRUCTURE.
//
// The rule of rnamotif_amd/csrc/rm_hitalign.h (what the widths and fill kernels of rm_hitalign_dev.hip compute) run on
// the CPU, for tests/test_hit_align_cpu.py and as the expected answer of tests/test_hit_align.py:
//
//   hit_align_check fill PROGRAM ENTRIES RECORDS OUT [WIDTHS [FILL]]
//     PROGRAM: the rma_program_t blob of a compiled descriptor; ENTRIES: int32 n, int32 slen[ n ], then the entries'
//     raw bytes one after the other; RECORDS: int32 records of the program's stride.  WIDTHS: "-" (what the records
//     need) or the columns' widths separated by commas; FILL: three bytes (default "-|.").  Writes OUT: int64
//     n_records, int64 W, int32 n_cols, int32 widths[ n_cols ], uint8 right[ n_cols ], uint8 rows[ n ][ W ], int32
//     pos[ n ][ W ].  Exit status 1 and "record H is bad" for a record hitwin_span refuses, "column C: width ..." for
//     a given width below what the records need.
//   hit_align_check check PROGRAM ENTRIES RECORDS -
//     one line per record: "code which" of rma::hitwin_span (ENTRIES may declare lengths only).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rm_hitalign.h"

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
	if( argc < 6 || argc > 8 ){
		fprintf( stderr, "usage: %s fill|check PROGRAM ENTRIES RECORDS OUT|- [WIDTHS [FILL]]\n", argv[ 0 ] );
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
	if( ent.size() >= 4 )
		memcpy( &n, ent.data(), 4 );
	if( n < 0 || ent.size() < 4 + size_t( n ) * 4 ){
		fprintf( stderr, "%s: no room for the lengths of %d entries\n", argv[ 3 ], n );
		return 2;
	}
	std::vector<int32_t>	slen( static_cast<size_t>( n ) );
	if( n > 0 )
		memcpy( slen.data(), ent.data() + 4, size_t( n ) * 4 );
	const std::vector<char>	rec_bytes = read_file( argv[ 4 ] );
	std::vector<int32_t>	recs( rec_bytes.size() / 4 );
	if( !recs.empty() )
		memcpy( recs.data(), rec_bytes.data(), recs.size() * 4 );
	const int	stride = rma_hit_stride( &prog );
	const int64_t	n_rec = int64_t( recs.size() ) / stride;
	const rma::HitWinShape	shape = rma::hitwin_shape( prog );

	if( mode == "check" ){
		for( int64_t h = 0; h < n_rec; h++ ){
			int32_t	lo, hi;
			int	which;
			const int	r = rma::hitwin_span( recs.data() + h * stride, shape, n, slen.data(), &lo, &hi, &which );
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
	// the check, then the widths over all records
	const int	nc = rma::hitalign_n_cols( shape );
	std::vector<int32_t>	need( static_cast<size_t>( nc ), 0 );
	for( int64_t h = 0; h < n_rec; h++ ){
		const int32_t	*w = recs.data() + h * stride;
		int32_t	lo, hi;
		int	which;
		if( rma::hitwin_span( w, shape, n, slen.data(), &lo, &hi, &which ) != rma::HW_OK ){
			fprintf( stderr, "record %lld is bad\n", ( long long )h );
			return 1;
		}
		for( int c = 0; c < nc; c++ ){
			const int32_t	f = rma::hitalign_width( w[ rma::hitstruct_word( shape, rma::hitalign_col_elem( shape, c ) ) + 1 ] );
			need[ c ] = f > need[ c ] ? f : need[ c ];
		}
	}
	std::vector<int32_t>	widths = need;
	if( argc > 6 && strcmp( argv[ 6 ], "-" ) ){
		widths.clear();
		for( const char *p = argv[ 6 ]; *p; ){
			char	*end;
			const long	v = strtol( p, &end, 10 );
			if( end == p || ( *end && *end != ',' ) ){
				fprintf( stderr, "WIDTHS: numbers separated by commas, not '%s'\n", argv[ 6 ] );
				return 2;
			}
			widths.push_back( int32_t( v ) );
			p = *end == ',' ? end + 1 : end;
		}
		if( int( widths.size() ) != nc ){
			fprintf( stderr, "%zu widths given, the descriptor has %d columns\n", widths.size(), nc );
			return 2;
		}
		for( int c = 0; c < nc; c++ )
			if( widths[ c ] < need[ c ] ){
				fprintf( stderr, "column %d: width %d given, the records need %d\n", c, widths[ c ], need[ c ] );
				return 1;
			}
	}
	uint8_t	fill[ 3 ] = { '-', '|', '.' };
	if( argc > 7 ){
		if( strlen( argv[ 7 ] ) != 3 ){
			fprintf( stderr, "FILL: three bytes\n" );
			return 2;
		}
		memcpy( fill, argv[ 7 ], 3 );
	}
	const rma::HitAlignLayout	lay = rma::hitalign_layout( prog, widths.data(), fill );
	const int64_t	W = lay.row_bytes;
	std::vector<uint8_t>	rows( size_t( n_rec * W ) );
	std::vector<int32_t>	pos( size_t( n_rec * W ) );
	for( int64_t h = 0; h < n_rec; h++ ){
		const int32_t	*w = recs.data() + h * stride;
		const int	e = w[ 0 ], comp = w[ 1 ];
		for( int64_t b = 0; b < W; b++ ){
			int32_t	p;
			const int	kind = rma::hitalign_byte( w, shape, lay, b, &p );
			uint8_t	v = rma::hitalign_fill_byte( lay.fill, kind );
			if( kind == rma::HA_LETTER ){
				const unsigned char	l = rma::hitwin_reader_letter( static_cast<unsigned char>( ent[ at[ e ] + size_t( rma::hitwin_src( comp, slen[ e ], p, 0 ) ) ] ) );
				v = comp ? rma::hitwin_wc_cmp( l ) : l;
			}
			rows[ size_t( h * W + b ) ] = v;
			pos[ size_t( h * W + b ) ] = p;
		}
	}
	FILE	*fp = fopen( argv[ 5 ], "wb" );
	if( fp == nullptr ){
		perror( argv[ 5 ] );
		return 2;
	}
	put( fp, std::vector<int64_t>{ n_rec, W } );
	put( fp, std::vector<int32_t>{ nc } );
	put( fp, widths );
	put( fp, std::vector<uint8_t>( lay.right, lay.right + nc ) );
	put( fp, rows );
	put( fp, pos );
	fclose( fp );
	return 0;
}
