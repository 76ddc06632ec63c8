// hit_ct_check.cpp -- TEST INFRASTRUCTURE.
//
// The rule of rnamotif_amd/csrc/rm_hitct.h (what the size and fill kernels of rm_hitct_dev.hip compute) run on the CPU,
// for tests/test_hit_ct_cpu.py and as the expected answer of tests/test_hit_ct.py:
//
//   hit_ct_check ct TYPE WORDS PROGRAM ENTRIES RECORDS NAMES SCORES OUT [ACCEPT]
//     TYPE: rnamotif or rnaviz; WORDS: the fields of the "#RM descr" line in one argument; the files as
//     hit_print_check.cpp takes them.  Writes OUT: int64 n_records, int64 off[ n_records + 1 ], the bytes.  Every
//     record's bytes are made line by line and counted by hitct_size(); hitct_byte() is asked for every byte of a record
//     of at most 400 bases and for every 97th of a longer one: exit status 3 where they disagree.  Exit status 1 with
//     hitct_table's words for a descriptor it refuses, and with "record H is bad: CODE" for a record hitprint_check or
//     hitct_measure refuses.
//   hit_ct_check energy
//     per line of stdin: the rule's "%.3f" of float( atof( line ) ) -- or "HC_NUMBER" --, a tab, and the C library's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rm_hitct.h"

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

static int energy_mode()
{
	char	line[ 4096 ];
	while( fgets( line, sizeof( line ), stdin ) != nullptr ){
		const size_t	n = strcspn( line, "\n" );
		line[ n ] = '\0';
		float	e = 0.0f;
		const uint8_t	*p = reinterpret_cast<const uint8_t *>( line );
		// (the byte behind the text is the NUL atof() stops at)
		const int	r = rma::hitct_energy( [ p ]( int64_t j ){ return p[ j ]; }, int64_t( n ), &e );
		if( r != rma::HW_OK )
			printf( "HC_NUMBER" );
		else{
			uint8_t	buf[ 64 ];
			RmsSink	o{ buf, 1, 0, int( sizeof( buf ) ), 0 };
			rma::hitct_fmt_energy( o, e );
			fwrite( buf, 1, size_t( o.n ), stdout );
		}
		printf( "\t%.3f\n", float( atof( line ) ) );
	}
	return 0;
}

int main( int argc, char **argv )
{
	if( argc == 2 && !strcmp( argv[ 1 ], "energy" ) )
		return energy_mode();
	if( argc < 10 || argc > 11 || strcmp( argv[ 1 ], "ct" ) || ( strcmp( argv[ 2 ], "rnamotif" ) && strcmp( argv[ 2 ], "rnaviz" ) ) ){
		fprintf( stderr, "usage: %s ct rnamotif|rnaviz WORDS PROGRAM ENTRIES RECORDS NAMES SCORES OUT [ACCEPT] | energy\n", argv[ 0 ] );
		return 2;
	}
	const int	type = !strcmp( argv[ 2 ], "rnaviz" ) ? rma::HC_RNAVIZ : rma::HC_RNAMOTIF;
	const std::vector<char>	blob = read_file( argv[ 4 ] );
	if( blob.size() != sizeof( rma_program_t ) ){
		fprintf( stderr, "%s: %zu bytes, a program has %zu\n", argv[ 4 ], blob.size(), sizeof( rma_program_t ) );
		return 2;
	}
	std::vector<rma_program_t>	progs( 1 );
	memcpy( progs.data(), blob.data(), sizeof( rma_program_t ) );
	const rma_program_t	&prog = progs[ 0 ];
	if( prog.magic != RMA_MAGIC || prog.size != sizeof( rma_program_t ) ){
		fprintf( stderr, "%s: not a program\n", argv[ 4 ] );
		return 2;
	}
	const rma::HitWinShape	shape = rma::hitwin_shape( prog );
	rma::HitCtTable	table;
	char	err[ 512 ];
	if( rma::hitct_table( argv[ 3 ], rma::hitalign_n_cols( shape ), &table, err, sizeof( err ) ) ){
		fprintf( stderr, "rm2ct: %s\n", err );
		return 1;
	}
	const std::vector<char>	ent = read_file( argv[ 5 ] );
	int32_t	n = 0;
	if( ent.size() >= 4 )
		memcpy( &n, ent.data(), 4 );
	if( n < 0 || ent.size() < 4 + size_t( n ) * 4 ){
		fprintf( stderr, "%s: no room for the lengths of %d entries\n", argv[ 5 ], n );
		return 2;
	}
	std::vector<int32_t>	slen( static_cast<size_t>( n ) );
	if( n > 0 )
		memcpy( slen.data(), ent.data() + 4, size_t( n ) * 4 );
	std::vector<size_t>	at( static_cast<size_t>( n ) );
	size_t	a = 4 + size_t( n ) * 4;
	for( int i = 0; i < n; i++ ){
		at[ i ] = a;
		a += size_t( slen[ i ] );
	}
	if( a > ent.size() ){
		fprintf( stderr, "%s: the entries' bytes end before the last entry does\n", argv[ 5 ] );
		return 2;
	}
	const std::vector<char>	rec_bytes = read_file( argv[ 6 ] );
	std::vector<int32_t>	recs( rec_bytes.size() / 4 );
	if( !recs.empty() )
		memcpy( recs.data(), rec_bytes.data(), recs.size() * 4 );
	const int	stride = rma_hit_stride( &prog );
	const int64_t	n_rec = int64_t( recs.size() ) / stride;
	const std::vector<char>	nm = read_file( argv[ 7 ] );
	std::vector<int64_t>	noff( 2 * size_t( n ) + 1 );
	if( nm.size() < noff.size() * 8 ){
		fprintf( stderr, "%s: no room for the offsets of %d names\n", argv[ 7 ], n );
		return 2;
	}
	memcpy( noff.data(), nm.data(), noff.size() * 8 );
	const uint8_t	*nbytes = reinterpret_cast<const uint8_t *>( nm.data() ) + noff.size() * 8;
	if( noff[ 0 ] != 0 || size_t( noff.back() ) != nm.size() - noff.size() * 8 ){
		fprintf( stderr, "%s: the offsets do not span the bytes\n", argv[ 7 ] );
		return 2;
	}
	const std::vector<char>	sc = read_file( argv[ 8 ] );
	int32_t	head[ 2 ] = { 0, 0 };
	if( sc.size() >= 8 )
		memcpy( head, sc.data(), 8 );
	const int32_t	width = head[ 1 ];
	if( sc.size() < 8 || head[ 0 ] != n_rec || width < 0 || sc.size() != 8 + size_t( n_rec ) * 4 + size_t( n_rec ) * size_t( width ) ){
		fprintf( stderr, "%s: not the score columns of %lld records\n", argv[ 8 ], ( long long )n_rec );
		return 2;
	}
	std::vector<int32_t>	text_len( static_cast<size_t>( n_rec ) );
	if( n_rec > 0 )
		memcpy( text_len.data(), sc.data() + 8, size_t( n_rec ) * 4 );
	const uint8_t	*text = reinterpret_cast<const uint8_t *>( sc.data() ) + 8 + size_t( n_rec ) * 4;
	std::vector<char>	accept;
	if( argc > 10 ){
		accept = read_file( argv[ 10 ] );
		if( int64_t( accept.size() ) != n_rec ){
			fprintf( stderr, "%s: %zu flags for %lld records\n", argv[ 10 ], accept.size(), ( long long )n_rec );
			return 2;
		}
	}
	std::vector<int64_t>	off( size_t( n_rec ) + 1, 0 );
	std::vector<uint8_t>	out;
	int32_t	pre[ rma::HC_PRE_ROOM ];
	for( int64_t h = 0; h < n_rec; h++ ){
		const int32_t	*w = recs.data() + h * stride;
		int	which;
		int	r = rma::hitprint_check( w, shape, n, slen.data(), text_len[ size_t( h ) ], width, &which );
		if( r != rma::HW_OK ){
			fprintf( stderr, "record %lld is bad: %d %d\n", ( long long )h, r, which );
			return 1;
		}
		const int	e = w[ 0 ];
		const rma::HitPrintIn	in{ noff[ 2 * size_t( e ) + 1 ] - noff[ 2 * size_t( e ) ], noff[ 2 * size_t( e ) + 2 ] - noff[ 2 * size_t( e ) + 1 ], slen[ e ],
			text_len[ size_t( h ) ] };
		uint8_t	num[ rma::HP_NUM_CAP ];
		const int	num_len = rma::hitprint_numbers( w, shape, in.slen, num, rma::HP_NUM_CAP );
		const Src	src{ nbytes + noff[ 2 * size_t( e ) ], nbytes + noff[ 2 * size_t( e ) + 1 ], text + size_t( h ) * size_t( width ), num,
			reinterpret_cast<const uint8_t *>( ent.data() ) + at[ size_t( e ) ], w[ 1 ], slen[ e ] };
		// (a record that is not accepted is not printed: the tool never sees its line)
		const bool	acc = accept.empty() || accept[ size_t( h ) ] != 0;
		float	energy = 0.0f;
		r = acc ? rma::hitct_measure( w, shape, in, type, num_len, src, &energy ) : int( rma::HW_OK );
		if( r != rma::HW_OK ){
			fprintf( stderr, "record %lld is bad: %d\n", ( long long )h, r );
			return 1;
		}
		rma::HitCtHead	hd{ 0, 0, 0, 0 };
		if( acc ){
			rma::hitct_prefix( w, shape, pre );
			hd = rma::hitct_head_of( w, shape, in.slen, pre[ table.n ] );
		}
		const int64_t	size = rma::hitct_size( type, table, pre, hd, energy, in.sid_len, acc );
		if( acc ){
			const size_t	first = out.size();
			uint8_t	buf[ 64 ];
			int	m = rma::hitct_head( type, hd, energy, buf, rma::HC_HEAD_CAP );
			bool	same = m <= rma::HC_HEAD_CAP;
			out.insert( out.end(), buf, buf + m );
			out.insert( out.end(), src.sid_p, src.sid_p + in.sid_len );
			m = rma::hitct_tail( type, hd, buf, rma::HC_TAIL_CAP );
			same = same && m <= rma::HC_TAIL_CAP;
			out.insert( out.end(), buf, buf + m );
			for( int32_t bn = 1; bn <= hd.nb; bn++ ){
				int	c;
				int32_t	k, pn;
				const int32_t	hn = rma::hitct_base( table.kind, table.mate, pre, table.n, hd, bn, &c, &k, &pn );
				const uint8_t	letter = src.letter( w[ rma::hitstruct_word( shape, rma::hitalign_col_elem( shape, c ) ) ] + k );
				m = rma::hitct_line( type, bn, hd.nb, letter, pn, hn, buf, rma::HC_LINE_CAP );
				same = same && m <= rma::HC_LINE_CAP && m == rma::hitct_line_len( bn, type, table.kind, table.mate, pre, table.n, hd );
				out.insert( out.end(), buf, buf + m );
			}
			same = same && int64_t( out.size() - first ) == size;
			const int64_t	step = hd.nb <= 400 ? 1 : 97;
			for( int64_t b = 0; same && b < size; b += step )
				same = rma::hitct_byte( type, table, w, shape, pre, hd, energy, in.sid_len, b, src ) == out[ first + size_t( b ) ];
			if( !same ){
				fprintf( stderr, "record %lld: hitct_size %lld, %zu bytes by lines, or hitct_byte differs\n", ( long long )h, ( long long )size,
					out.size() - first );
				return 3;
			}
		}else if( size != 0 ){
			fprintf( stderr, "record %lld: not accepted, hitct_size %lld\n", ( long long )h, ( long long )size );
			return 3;
		}
		off[ size_t( h ) + 1 ] = int64_t( out.size() );
	}
	FILE	*fp = fopen( argv[ 9 ], "wb" );
	if( fp == nullptr ){
		perror( argv[ 9 ] );
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
