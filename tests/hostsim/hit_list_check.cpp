// hit_list_check.cpp -- TEST INFRASTRUCTURE.
//
// The rule of rnamotif_amd/csrc/rm_hitlist.h (what the kernels of rm_hitlist_dev.hip compute) run on the CPU with
// std::sort under rmlist_less, for tests/test_hit_list_cpu.py and as the expected answer of tests/test_hit_list.py:
//
//   hit_list_check list PROGRAM ENTRIES RECORDS NAMES SCORES OUT NAME_MODE SMAX ACCEPT|- WIDTHS|- [LETTERS]
//     PROGRAM, ENTRIES, RECORDS, NAMES, SCORES, ACCEPT: as hit_print_check takes them; NAME_MODE: 0 whole, 1 locus,
//     2 accession; SMAX: <= 0 for rmfmt's 30000000; WIDTHS: the segments' widths as "w,w,..." to lay the lines out with
//     instead of the widest instances; LETTERS: a file of 256 bytes, the letter of every text byte (default: the
//     readers').  Writes OUT: int64 n_lines, int64 line_len, int64 temp_bytes, int32 mode, int32 n_segs,
//     int32 width[ n_segs ], int64 perm[ n_lines ], the n_lines * line_len bytes.  Every line is made twice, cell by
//     cell and by rmlist_line_byte(): exit status 3 where they disagree or a line's length is not line_len, or where
//     rmlist_temp_byte() does not give temp_len bytes that end in a newline.
//     Exit status 1 and the words of the refusal for records the rule refuses.
//   hit_list_check order ... (the same arguments)
//     Writes OUT: int64 n (the printed records), int32 mode, int32 0, int64 index[ n ], uint8 less[ n ][ n ] -- rmlist_less
//     of every pair under the listing's mode (mode 0: under mode 2) --, then the n temp lines.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rm_hitlist.h"

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

// the letters of one record's strand
struct Let {
	const uint8_t	*entry_p, *table;
	int32_t	comp, slen;
	uint8_t	letter( int32_t p ) const
	{
		const unsigned char	l = table[ entry_p[ rma::hitwin_src( comp, slen, p, 0 ) ] ];
		return comp ? rma::hitwin_wc_cmp( l ) : l;
	}
};
typedef rma::HitListView<Let>	View;

int main( int argc, char **argv )
{
	const char	*who = "hit_list_check";
	if( argc < 12 || argc > 13 ){
		fprintf( stderr, "usage: %s list|order PROGRAM ENTRIES RECORDS NAMES SCORES OUT NAME_MODE SMAX ACCEPT|- WIDTHS|- [LETTERS]\n", argv[ 0 ] );
		return 2;
	}
	const std::string	what = argv[ 1 ];
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
	const std::vector<char>	rec_bytes = read_file( argv[ 4 ] );
	std::vector<int32_t>	recs( rec_bytes.size() / 4 );
	if( !recs.empty() )
		memcpy( recs.data(), rec_bytes.data(), recs.size() * 4 );
	const int	stride = rma_hit_stride( &prog );
	const int64_t	n_rec = int64_t( recs.size() ) / stride;
	const rma::HitWinShape	shape = rma::hitwin_shape( prog );
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
	const int	name_mode = atoi( argv[ 8 ] );
	const int64_t	smax = atoll( argv[ 9 ] ) > 0 ? atoll( argv[ 9 ] ) : rma::HL_SMAX;
	std::vector<char>	accept;
	if( strcmp( argv[ 10 ], "-" ) ){
		accept = read_file( argv[ 10 ] );
		if( int64_t( accept.size() ) != n_rec ){
			fprintf( stderr, "%s: %zu flags for %lld records\n", argv[ 10 ], accept.size(), ( long long )n_rec );
			return 2;
		}
	}
	uint8_t	table[ 256 ];
	for( int b = 0; b < 256; b++ )
		table[ b ] = rma::hitwin_reader_letter( static_cast<unsigned char>( b ) );
	if( argc > 12 ){
		const std::vector<char>	t = read_file( argv[ 12 ] );
		if( t.size() != 256 ){
			fprintf( stderr, "%s: %zu bytes, a letters table has 256\n", argv[ 12 ], t.size() );
			return 2;
		}
		memcpy( table, t.data(), 256 );
	}
	char	err[ 512 ];
	// what the call refuses before it looks at a record
	for( int b = 0; b < 256; b++ )
		if( table[ b ] == ' ' || table[ b ] == '\t' || table[ b ] == '\n' ){
			fprintf( stderr, "%s: the letters map byte %d to a blank, a tab or a newline: nothing listed\n", who, b );
			return 1;
		}
	for( int e = 0; e < n; e++ ){
		const int64_t	m = noff[ 2 * size_t( e ) + 1 ] - noff[ 2 * size_t( e ) ];
		const uint8_t	*sid = nbytes + noff[ 2 * size_t( e ) ];
		int32_t	nat;
		bool	bad = rma::rmlist_name( sid, int32_t( m ), name_mode, &nat ) == 0;
		for( int64_t j = 0; j < m; j++ )
			bad = bad || sid[ j ] == ' ' || sid[ j ] == '\t' || sid[ j ] == '\n';
		if( bad ){
			fprintf( stderr, "%s: entry %d: its name is empty, trims to nothing or has a blank, a tab or a newline in it: rmfmt would split the line there: nothing listed\n", who, e );
			return 1;
		}
	}

	// measure
	const int	n_segs = rma::rmlist_n_segs( shape );
	std::vector<rma::HitListRec>	meas( static_cast<size_t>( n_rec ) );
	std::vector<View>	views( static_cast<size_t>( n_rec ) );
	std::vector<int64_t>	perm;
	std::vector<int32_t>	widths( size_t( n_segs ), 0 );
	int64_t	temp_bytes = 0;
	bool	scored = true;
	for( int64_t h = 0; h < n_rec; h++ ){
		const int32_t	*w = recs.data() + h * stride;
		int	which;
		const int	r = rma::hitprint_check( w, shape, n, slen.data(), text_len[ size_t( h ) ], width, &which );
		if( r != rma::HW_OK ){
			fprintf( stderr, "record %lld is bad: %d %d\n", ( long long )h, r, which );
			return 1;
		}
		rma::HitListRec	&m = meas[ size_t( h ) ];
		m.k = -1;
		if( !accept.empty() && accept[ size_t( h ) ] == 0 )
			continue;
		const size_t	e = size_t( w[ 0 ] );
		const rma::HitPrintIn	in{ noff[ 2 * e + 1 ] - noff[ 2 * e ], noff[ 2 * e + 2 ] - noff[ 2 * e + 1 ], slen[ e ], text_len[ size_t( h ) ] };
		const uint8_t	*sid = nbytes + noff[ 2 * e ], *col = text + size_t( h ) * size_t( width );
		const int	c = rma::rmlist_measure( w, shape, in, sid, col, name_mode, &m );
		if( c != rma::HW_OK ){
			rma::rmlist_refusal( err, sizeof( err ), who, c, ( long long )h );
			fprintf( stderr, "%s\n", err );
			return 1;
		}
		if( !perm.empty() && meas[ size_t( perm[ 0 ] ) ].k != m.k ){
			rma::rmlist_refusal_mixed( err, sizeof( err ), who, ( long long )perm[ 0 ], meas[ size_t( perm[ 0 ] ) ].k, ( long long )h, m.k );
			fprintf( stderr, "%s\n", err );
			return 1;
		}
		views[ size_t( h ) ] = View{ &m, w, sid, col, in.text_len, Let{ reinterpret_cast<const uint8_t *>( ent.data() ) + at[ e ], table, w[ 1 ], slen[ e ] } };
		perm.push_back( h );
		temp_bytes += m.temp_len;
		scored = scored && ( m.flags & rma::HL_F_NUMBER );
		for( int g = 0; g < n_segs; g++ )
			widths[ size_t( g ) ] = std::max( widths[ size_t( g ) ], rma::rmlist_seg_len( m, w, shape, g ) );
	}
	const int	mode = temp_bytes > smax ? 0 : scored ? 1 : 2;
	const int64_t	n_lines = int64_t( perm.size() );
	const int	k = n_lines > 0 ? meas[ size_t( perm[ 0 ] ) ].k : 1;

	// the temp lines, by rmlist_temp_byte
	std::vector<std::string>	temp( static_cast<size_t>( n_lines ) );
	for( int64_t i = 0; i < n_lines; i++ ){
		const View	&v = views[ size_t( perm[ size_t( i ) ] ) ];
		for( int32_t b = 0; b < v.r->temp_len; b++ )
			temp[ size_t( i ) ].push_back( char( rma::rmlist_temp_byte( v, shape, b ) ) );
		const std::string	&t = temp[ size_t( i ) ];
		if( t.empty() || t.back() != '\n' || t.find( '\n' ) != t.size() - 1 ){
			fprintf( stderr, "record %lld: rmlist_temp_byte does not give a line of temp_len %d bytes\n", ( long long )perm[ size_t( i ) ], v.r->temp_len );
			return 3;
		}
	}
	FILE	*fp = fopen( argv[ 7 ], "wb" );
	if( fp == nullptr ){
		perror( argv[ 7 ] );
		return 2;
	}
	if( what == "order" ){
		const int32_t	hd[ 2 ] = { mode, 0 };
		std::vector<uint8_t>	less( size_t( n_lines ) * size_t( n_lines ) );
		for( int64_t i = 0; i < n_lines; i++ )
			for( int64_t j = 0; j < n_lines; j++ )
				less[ size_t( i * n_lines + j ) ] = rma::rmlist_less( mode == 0 ? 2 : mode, shape, views[ size_t( perm[ size_t( i ) ] ) ], perm[ size_t( i ) ],
					views[ size_t( perm[ size_t( j ) ] ) ], perm[ size_t( j ) ] ) ? 1 : 0;
		fwrite( &n_lines, 8, 1, fp );
		fwrite( hd, 4, 2, fp );
		fwrite( perm.data(), 8, perm.size(), fp );
		fwrite( less.data(), 1, less.size(), fp );
		for( const std::string &t : temp )
			fwrite( t.data(), 1, t.size(), fp );
		fclose( fp );
		return 0;
	}
	if( mode != 0 )
		std::sort( perm.begin(), perm.end(), [ & ]( int64_t x, int64_t y ){
			return rma::rmlist_less( mode, shape, views[ size_t( x ) ], x, views[ size_t( y ) ], y );
		} );
	if( strcmp( argv[ 11 ], "-" ) ){
		int	g = 0;
		for( const char *p = argv[ 11 ]; *p && g < n_segs; g++ ){
			widths[ size_t( g ) ] = atoi( p );
			p += strcspn( p, "," );
			p += *p == ',';
		}
	}
	uint8_t	right[ rma::HA_MAX_COLS ];
	rma::hitalign_directions( prog, right );
	const rma::HitListLayout	lay = rma::rmlist_layout( shape, right, widths.data(), k );
	std::vector<uint8_t>	out;
	for( int64_t i = 0; i < n_lines; i++ ){
		const int64_t	h = perm[ size_t( i ) ];
		const View	&v = views[ size_t( h ) ];
		// cell by cell: the text, padded on the side the column asks for
		std::string	line;
		for( int g = 0; g < n_segs; g++ ){
			std::string	t;
			for( int32_t j = 0; j < rma::rmlist_seg_len( *v.r, v.w, shape, g ); j++ )
				t.push_back( char( rma::rmlist_seg_byte( v, shape, g, j ) ) );
			const std::string	pad( size_t( std::max<int64_t>( 0, int64_t( lay.width[ g ] ) - int64_t( t.size() ) ) ), ' ' );
			line += ( g > 0 ? " " : "" ) + ( lay.right[ g ] ? pad + t : t + pad );
		}
		line += "\n";
		bool	same = int64_t( line.size() ) == lay.line_len;
		for( int32_t b = 0; same && b < lay.line_len; b++ )
			same = rma::rmlist_line_byte( v, shape, lay, b ) == uint8_t( line[ size_t( b ) ] );
		if( !same ){
			fprintf( stderr, "record %lld: a line of %zu bytes, line_len is %d, or rmlist_line_byte differs\n", ( long long )h, line.size(), lay.line_len );
			return 3;
		}
		out.insert( out.end(), line.begin(), line.end() );
	}
	const int64_t	hd64[ 3 ] = { n_lines, lay.line_len, temp_bytes };
	const int32_t	hd32[ 2 ] = { mode, n_segs };
	if( fwrite( hd64, 8, 3, fp ) != 3 || fwrite( hd32, 4, 2, fp ) != 2 || fwrite( widths.data(), 4, widths.size(), fp ) != widths.size() ||
		( !perm.empty() && fwrite( perm.data(), 8, perm.size(), fp ) != perm.size() ) ||
		( !out.empty() && fwrite( out.data(), 1, out.size(), fp ) != out.size() ) ){
		perror( "write" );
		return 2;
	}
	fclose( fp );
	return 0;
}
