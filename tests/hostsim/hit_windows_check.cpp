// hit_windows_check.cpp -- TEST INFRASTRUCTURE.
//
// The window rule of rnamotif_amd/csrc/rm_hitwin.h (what the kernels of rm_hitwin_dev.hip cut out of a device
// database's text) against the host's own ways of rebuilding a hit's text, on the CPU (tests/test_hit_windows_cpu.py):
//
//   hit_windows_check replay ENTRIES RECORDS OUTDIR [rnamotif options] -descr file.descr
//     ENTRIES: int32 n, int32 slen[ n ], then the entries' raw bytes one after the other; RECORDS: int32 records of
//     the descriptor's stride.  The entries normalised by the readers' rule are replayed three times, each with a
//     descriptor of its own: Replayer::replay (whole strands, revcomp()) into OUTDIR/replay.out,
//     Replayer::replay_packed (PackFile::window) into OUTDIR/packed.out, and Replayer::replay_windows over windows
//     made from the raw bytes by rm_hitwin.h, handed over in pieces of 1 to 7 records, into OUTDIR/windows.out.
//     Every window is also compared with PackFile::window.  Prints "records R hits H accepted A mismatches M".
//   hit_windows_check span ENTRIES RECORDS - [rnamotif options] -descr file.descr
//     one line per record: "code lo hi which" of rma::hitwin_span.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rm_cli.h"
#include "rm_driver.h"
#include "rm_hitwin.h"
#include "rm_pack.h"

static std::vector<char> read_file( const std::string &path )
{
	std::vector<char>	v;
	FILE	*fp = fopen( path.c_str(), "rb" );
	if( fp == nullptr ){
		perror( path.c_str() );
		exit( 2 );
	}
	char	buf[ 65536 ];
	size_t	n;
	while( ( n = fread( buf, 1, sizeof( buf ), fp ) ) > 0 )
		v.insert( v.end(), buf, buf + n );
	fclose( fp );
	return v;
}

static rma::Prepared prepared( std::vector<char *> &args )
{
	return rma::prepare( rma::parse_args( int( args.size() ), args.data() ) );
}

int main( int argc, char **argv )
{
	if( argc < 6 ){
		fprintf( stderr, "usage: %s replay|span ENTRIES RECORDS OUTDIR|- [rnamotif options] -descr file\n", argv[ 0 ] );
		return 2;
	}
	const std::string	mode = argv[ 1 ], outdir = argv[ 4 ];
	std::vector<char *>	args{ argv[ 0 ] };
	for( int i = 5; i < argc; i++ )
		args.push_back( argv[ i ] );
	// the entries, raw and as the readers deliver them
	const std::vector<char>	ent = read_file( argv[ 2 ] );
	int32_t	n = 0;
	memcpy( &n, ent.data(), 4 );
	std::vector<int32_t>	slen( static_cast<size_t>( n ) );
	memcpy( slen.data(), ent.data() + 4, size_t( n ) * 4 );
	const std::vector<char>	rec_bytes = read_file( argv[ 3 ] );
	std::vector<int32_t>	recs( rec_bytes.size() / 4 );
	memcpy( recs.data(), rec_bytes.data(), recs.size() * 4 );

	rma::Prepared	p1 = prepared( args );
	const rma_program_t	&prog = *p1.prog;
	const int	stride = rma_hit_stride( &prog );
	const int64_t	n_rec = int64_t( recs.size() ) / stride;
	const rma::HitWinShape	shape = rma::hitwin_shape( prog );

	if( mode == "span" ){
		for( int64_t h = 0; h < n_rec; h++ ){
			int32_t	lo, hi;
			int	which;
			const int	r = rma::hitwin_span( recs.data() + h * stride, shape, n, slen.data(), &lo, &hi, &which );
			printf( "%d %d %d %d\n", r, lo, hi, which );
		}
		return 0;
	}
	// (span mode declares lengths only)
	std::vector<std::string>	raw;
	std::vector<rma::SeqRecord>	batch( static_cast<size_t>( n ) );
	size_t	at = 4 + size_t( n ) * 4;
	for( int i = 0; i < n; i++ ){
		if( at + size_t( slen[ i ] ) > ent.size() ){
			fprintf( stderr, "entry %d: %d bytes past the end of the file\n", i, slen[ i ] );
			return 2;
		}
		raw.emplace_back( ent.data() + at, size_t( slen[ i ] ) );
		at += size_t( slen[ i ] );
		batch[ i ].sid = "e" + std::to_string( i );
		batch[ i ].sdef = "entry " + std::to_string( i );
		for( char c : raw.back() )
			batch[ i ].seq.push_back( char( rma::hitwin_reader_letter( static_cast<unsigned char>( c ) ) ) );
	}

	// the windows by the rule: letters of the raw bytes, strand 1 from the 3' end, complemented
	std::vector<char>	windows;
	std::vector<int64_t>	off{ 0 };
	std::vector<int32_t>	lo_of;
	int64_t	mismatches = 0;
	rma::PackFile	pk;
	for( const rma::SeqRecord &r : batch )
		pk.add( r );
	std::vector<char>	want;
	for( int64_t h = 0; h < n_rec; h++ ){
		const int32_t	*w = recs.data() + h * stride;
		int32_t	lo, hi;
		int	which;
		if( rma::hitwin_span( w, shape, n, slen.data(), &lo, &hi, &which ) != rma::HW_OK ){
			fprintf( stderr, "record %lld is bad\n", ( long long )h );
			return 1;
		}
		const int	e = w[ 0 ], comp = w[ 1 ];
		const int64_t	m = rma::hitwin_len( lo, hi );
		want.assign( size_t( slen[ e ] ) + 1, '?' );
		pk.window( e, comp, lo, hi, want.data() );
		for( int64_t i = 0; i < m; i++ ){
			const unsigned char	l = rma::hitwin_reader_letter( static_cast<unsigned char>( raw[ e ][ size_t( rma::hitwin_src( comp, slen[ e ], lo, i ) ) ] ) );
			const char	c = char( comp ? rma::hitwin_wc_cmp( l ) : l );
			windows.push_back( c );
			if( c != want[ size_t( lo + i ) ] )
				mismatches++;
		}
		off.push_back( int64_t( windows.size() ) );
		lo_of.push_back( lo );
	}

	// three replays
	auto open = [ & ]( const char *name ) -> FILE * {
		FILE	*fp = fopen( ( outdir + "/" + name ).c_str(), "w" );
		if( fp == nullptr ){
			perror( name );
			exit( 2 );
		}
		return fp;
	};
	rma::SearchStats	s1, s2, s3;
	{
		FILE	*fp = open( "replay.out" );
		rma::Replayer	r( *p1.descr, prog, fp );
		r.begin();
		r.replay( batch, recs.data(), n_rec, s1 );
		r.end();
		fclose( fp );
	}
	{
		rma::Prepared	p2 = prepared( args );
		FILE	*fp = open( "packed.out" );
		rma::Replayer	r( *p2.descr, *p2.prog, fp );
		r.begin();
		r.replay_packed( pk, 0, recs.data(), n_rec, s2 );
		r.end();
		fclose( fp );
	}
	std::vector<uint8_t>	accepted( static_cast<size_t>( std::max<int64_t>( n_rec, 1 ) ), 7 );
	{
		rma::Prepared	p3 = prepared( args );
		FILE	*fp = open( "windows.out" );
		rma::Replayer	r( *p3.descr, *p3.prog, fp );
		r.begin();
		std::vector<const char *>	sids, sdefs;
		for( const rma::SeqRecord &b : batch ){
			sids.push_back( b.sid.c_str() );
			sdefs.push_back( b.sdef.c_str() );
		}
		// pieces of 1 to 7 records, their offsets from their own first window, as rma_replay_device hands them on
		std::vector<int64_t>	poff;
		for( int64_t a = 0, k = 0; a < n_rec; k++ ){
			const int64_t	b = std::min( n_rec, a + 1 + k % 7 );
			poff.clear();
			for( int64_t i = a; i <= b; i++ )
				poff.push_back( off[ size_t( i ) ] - off[ size_t( a ) ] );
			r.replay_windows( recs.data() + a * stride, b - a, windows.data() + off[ size_t( a ) ], poff.data(), lo_of.data() + a,
				slen.data(), n, sids.data(), sdefs.data(), accepted.data() + a, s3 );
			a = b;
		}
		r.end();
		fclose( fp );
	}
	int64_t	n_acc = 0;
	for( int64_t h = 0; h < n_rec; h++ ){
		if( accepted[ size_t( h ) ] > 1 ){
			fprintf( stderr, "accepted[ %lld ] not written\n", ( long long )h );
			return 1;
		}
		n_acc += accepted[ size_t( h ) ];
	}
	if( s1.n_hits != s2.n_hits || s1.n_hits != s3.n_hits || s1.n_candidates != s3.n_candidates ){
		fprintf( stderr, "hits %lld / %lld / %lld, candidates %lld / %lld\n", ( long long )s1.n_hits, ( long long )s2.n_hits,
			( long long )s3.n_hits, ( long long )s1.n_candidates, ( long long )s3.n_candidates );
		return 1;
	}
	printf( "records %lld hits %lld accepted %lld mismatches %lld\n", ( long long )n_rec, ( long long )s3.n_hits, ( long long )n_acc,
		( long long )mismatches );
	return 0;
}
