// hit_print_check.cpp -- TEST INFRASTRUCTURE.
//
// The rule of rnamotif_amd/csrc/rm_hitprint.h (what the size and fill kernels of rm_hitprint_dev.hip compute) run on
// the CPU, for tests/test_hit_print_cpu.py and as the expected answer of tests/test_hit_print.py:
//
//   hit_print_check print PROGRAM ENTRIES RECORDS NAMES SCORES OUT [ACCEPT]
//     PROGRAM: the rma_program_t blob of a compiled descriptor; ENTRIES: int32 n, int32 slen[ n ], then the entries'
//     raw bytes one after the other; RECORDS: int32 records of the program's stride; NAMES: int64 off[ 2 n + 1 ], then
//     the bytes (entry e: its sid at [ off[ 2e ], off[ 2e + 1 ] ), its sdef behind it); SCORES: int32 n_records, int32
//     width, int32 text_len[ n_records ], uint8 text[ n_records ][ width ]; ACCEPT: a byte per record (default: all).
//     Writes OUT: int64 n_records, int64 off[ n_records + 1 ], the bytes.  Every record's bytes are made twice, by the
//     segments in turn and by hitprint_byte(), and counted by hitprint_size(): exit status 3 where the three disagree.
//     Exit status 1 and "record H is bad: CODE WHICH" for a record hitprint_check refuses.
//   hit_print_check check PROGRAM ENTRIES RECORDS - SCORES -
//     one line per record: "code which" of rma::hitprint_check (ENTRIES may declare lengths only).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rm_hitprint.h"

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

// what hitprint_seg_byte reads, for one record
struct Src {
	const uint8_t	*sid_p, *sdef_p, *score_p, *num_p, *entry_p;
	int32_t	comp, slen;
	uint8_t	sid( int64_t j ) const { return sid_p[ j ]; }
	uint8_t	sdef( int64_t j ) const { return sdef_p[ j ]; }
	uint8_t	score( int64_t j ) const { return score_p[ j ]; }
	uint8_t	num( int64_t j ) const { return num_p[ j ]; }
	uint8_t	letter( int32_t p ) const
	{
		const unsigned char	l = rma::hitwin_reader_letter( entry_p[ rma::hitwin_src( comp, slen, p, 0 ) ] );
		return comp ? rma::hitwin_wc_cmp( l ) : l;
	}
};

int main( int argc, char **argv )
{
	if( argc < 8 || argc > 9 ){
		fprintf( stderr, "usage: %s print|check PROGRAM ENTRIES RECORDS NAMES|- SCORES OUT|- [ACCEPT]\n", argv[ 0 ] );
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
	// the score columns
	const std::vector<char>	sc = read_file( argv[ 6 ] );
	int32_t	head[ 2 ] = { 0, 0 };
	if( sc.size() >= 8 )
		memcpy( head, sc.data(), 8 );
	const int32_t	width = head[ 1 ];
	if( sc.size() < 8 || head[ 0 ] != n_rec || width < 0 || sc.size() != 8 + size_t( n_rec ) * 4 + size_t( n_rec ) * size_t( width ) ){
		fprintf( stderr, "%s: not the score columns of %lld records\n", argv[ 6 ], ( long long )n_rec );
		return 2;
	}
	std::vector<int32_t>	text_len( static_cast<size_t>( n_rec ) );
	if( n_rec > 0 )
		memcpy( text_len.data(), sc.data() + 8, size_t( n_rec ) * 4 );
	const uint8_t	*text = reinterpret_cast<const uint8_t *>( sc.data() ) + 8 + size_t( n_rec ) * 4;

	if( mode == "check" ){
		for( int64_t h = 0; h < n_rec; h++ ){
			int	which;
			const int	r = rma::hitprint_check( recs.data() + h * stride, shape, n, slen.data(), text_len[ size_t( h ) ], width, &which );
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
	const std::vector<char>	nm = read_file( argv[ 5 ] );
	std::vector<int64_t>	noff( 2 * size_t( n ) + 1 );
	if( nm.size() < noff.size() * 8 ){
		fprintf( stderr, "%s: no room for the offsets of %d names\n", argv[ 5 ], n );
		return 2;
	}
	memcpy( noff.data(), nm.data(), noff.size() * 8 );
	const uint8_t	*nbytes = reinterpret_cast<const uint8_t *>( nm.data() ) + noff.size() * 8;
	if( noff[ 0 ] != 0 || size_t( noff.back() ) != nm.size() - noff.size() * 8 ){
		fprintf( stderr, "%s: the offsets do not span the bytes\n", argv[ 5 ] );
		return 2;
	}
	std::vector<char>	accept;
	if( argc > 8 ){
		accept = read_file( argv[ 8 ] );
		if( int64_t( accept.size() ) != n_rec ){
			fprintf( stderr, "%s: %zu flags for %lld records\n", argv[ 8 ], accept.size(), ( long long )n_rec );
			return 2;
		}
	}
	std::vector<int64_t>	off( size_t( n_rec ) + 1, 0 );
	std::vector<uint8_t>	out;
	for( int64_t h = 0; h < n_rec; h++ ){
		const int32_t	*w = recs.data() + h * stride;
		int	which;
		const int	r = rma::hitprint_check( w, shape, n, slen.data(), text_len[ size_t( h ) ], width, &which );
		if( r != rma::HW_OK ){
			fprintf( stderr, "record %lld is bad: %d %d\n", ( long long )h, r, which );
			return 1;
		}
		const int	e = w[ 0 ];
		const rma::HitPrintIn	in{ noff[ 2 * size_t( e ) + 1 ] - noff[ 2 * size_t( e ) ], noff[ 2 * size_t( e ) + 2 ] - noff[ 2 * size_t( e ) + 1 ], slen[ e ],
			text_len[ size_t( h ) ] };
		const bool	acc = accept.empty() || accept[ size_t( h ) ] != 0;
		const int64_t	size = rma::hitprint_size( w, shape, in, acc );
		if( acc ){
			uint8_t	num[ rma::HP_NUM_CAP ];
			const int	num_len = rma::hitprint_numbers( w, shape, in.slen, num, rma::HP_NUM_CAP );
			const Src	src{ nbytes + noff[ 2 * size_t( e ) ], nbytes + noff[ 2 * size_t( e ) + 1 ], text + size_t( h ) * size_t( width ), num,
				reinterpret_cast<const uint8_t *>( ent.data() ) + at[ size_t( e ) ], w[ 1 ], slen[ e ] };
			const size_t	first = out.size();
			for( int k = 0; k < rma::hitprint_n_segs( shape ); k++ ){
				const rma::HitPrintSeg	g = rma::hitprint_seg( w, shape, in, num_len, k );
				for( int64_t j = 0; j < g.len; j++ )
					out.push_back( rma::hitprint_seg_byte( w, g, j, src ) );
			}
			bool	same = int64_t( out.size() - first ) == size && num_len <= rma::HP_NUM_CAP;
			for( int64_t b = 0; same && b < size; b++ )
				same = rma::hitprint_byte( w, shape, in, num_len, b, src ) == out[ first + size_t( b ) ];
			if( !same ){
				fprintf( stderr, "record %lld: hitprint_size %lld, %zu bytes by segments, or hitprint_byte differs\n", ( long long )h,
					( long long )size, out.size() - first );
				return 3;
			}
		}else if( size != 0 ){
			fprintf( stderr, "record %lld: not accepted, hitprint_size %lld\n", ( long long )h, ( long long )size );
			return 3;
		}
		off[ size_t( h ) + 1 ] = int64_t( out.size() );
	}
	FILE	*fp = fopen( argv[ 7 ], "wb" );
	if( fp == nullptr ){
		perror( argv[ 7 ] );
		return 2;
	}
	const int64_t	count = n_rec;
	if( fwrite( &count, 8, 1, fp ) != 1 || fwrite( off.data(), 8, off.size(), fp ) != off.size() ||
		( !out.empty() && fwrite( out.data(), 1, out.size(), fp ) != out.size() ) ){
		perror( "write" );
		return 2;
	}
	fclose( fp );
	return 0;
}
