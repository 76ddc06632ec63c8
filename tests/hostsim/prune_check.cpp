// prune_check.cpp -- TEST INFRASTRUCTURE.
//
// The rule of rnamotif_amd/csrc/rm_prune.h (what the kernels of rm_prune_dev.hip decide per hit record) run on the
// CPU, for tests/test_prune_cpu.py and as the expected answer of tests/test_prune.py:
//
//   prune_check mask PROGRAM ENTRIES RECORDS GROUPS|-
//     PROGRAM: the rma_program_t blob of a compiled descriptor; ENTRIES: int32 n, int32 slen[ n ] (anything behind
//     them is not read); RECORDS: int32 records of the program's stride; GROUPS: int32 group_of_entry[ n ], or "-"
//     for every entry its own.  Prints the mask as one line of 0 / 1, then "down D left L blocks B groups G": the
//     records dropped via DOWN and via LEFT, the blocks and the groups of the pass.  Exit status 1 and
//     "record H is bad" for a record hitwin_span refuses.
//   prune_check table PROGRAM
//     one line per printed field: its kind (the tool's K_* number) and its group's printed-field indices.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rm_prune.h"

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

int main( int argc, char **argv )
{
	const std::string	mode = argc > 1 ? argv[ 1 ] : "";
	if( !( ( mode == "mask" && argc == 6 ) || ( mode == "table" && argc == 3 ) ) ){
		fprintf( stderr, "usage: %s mask PROGRAM ENTRIES RECORDS GROUPS|-\n       %s table PROGRAM\n", argv[ 0 ], argv[ 0 ] );
		return 2;
	}
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
	if( mode == "table" ){
		const rma::PruneTable	t = rma::prune_table( prog );
		for( int f = 0; f < t.n_fields; f++ ){
			printf( "%d", t.kind[ f ] );
			for( int i = 0; i < 4 && t.group[ f ][ i ] >= 0; i++ )
				printf( " %d", t.group[ f ][ i ] );
			printf( "\n" );
		}
		return 0;
	}
	const std::vector<char>	ent = read_file( argv[ 3 ] );
	int32_t	n = 0;
	if( ent.size() >= 4 )
		memcpy( &n, ent.data(), 4 );
	if( n < 0 || ent.size() < 4 + size_t( n ) * 4 ){
		fprintf( stderr, "%s: not the entries' lengths\n", argv[ 3 ] );
		return 2;
	}
	std::vector<int32_t>	slen( static_cast<size_t>( n ) );
	if( n > 0 )
		memcpy( slen.data(), ent.data() + 4, size_t( n ) * 4 );
	const std::vector<char>	rec_bytes = read_file( argv[ 4 ] );
	std::vector<int32_t>	recs( rec_bytes.size() / 4 );
	if( !recs.empty() )
		memcpy( recs.data(), rec_bytes.data(), recs.size() * 4 );
	std::vector<int32_t>	groups;
	if( strcmp( argv[ 5 ], "-" ) != 0 ){
		const std::vector<char>	g = read_file( argv[ 5 ] );
		if( g.size() != size_t( n ) * 4 ){
			fprintf( stderr, "%s: %zu bytes, one int32 per entry is %zu\n", argv[ 5 ], g.size(), size_t( n ) * 4 );
			return 2;
		}
		groups.resize( size_t( n ) );
		if( n > 0 )
			memcpy( groups.data(), g.data(), g.size() );
	}
	const int	stride = rma_hit_stride( &prog );
	const int64_t	n_rec = int64_t( recs.size() ) / stride;
	std::vector<uint8_t>	keep( size_t( n_rec ) + 1 );
	rma::PruneCounts	c;
	const int64_t	bad = rma::prune_mask( recs.data(), n_rec, stride, prog, n, slen.data(), strcmp( argv[ 5 ], "-" ) != 0 ? groups.data() : nullptr,
		keep.data(), &c );
	if( bad >= 0 ){
		fprintf( stderr, "record %lld is bad\n", ( long long )bad );
		return 1;
	}
	std::string	line( size_t( n_rec ), '0' );
	for( int64_t h = 0; h < n_rec; h++ )
		line[ size_t( h ) ] = keep[ size_t( h ) ] ? '1' : '0';
	printf( "%s\ndown %lld left %lld blocks %lld groups %lld\n", line.c_str(), ( long long )c.down, ( long long )c.left, ( long long )c.blocks,
		( long long )c.groups );
	return 0;
}
