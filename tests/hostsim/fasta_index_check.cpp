// fasta_index_check.cpp -- TEST INFRASTRUCTURE.
//
// The rule the device route reads FASTA text by (rnamotif_amd/csrc/rm_fasta_dev.h: chunk summaries, their
// scan, the pass that applies it) run on the host, chunk by chunk as the kernels run it, against the parallel
// reader (FastaStream, rm_stream.cpp) on the same bytes: the entries' starts, the ends of their definition
// lines, their letters and lengths, their names and definitions, and whether (and at which entry) the text is
// refused.
//
//   fasta_index_check files  maxslen chunks file...   chunks: comma separated, 0 = FD_CHUNK; maxslen as FastaStream's
//   fasta_index_check compose n seed                  n random triples of summaries composed both ways
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "rm_fasta_dev.h"
#include "rm_stream.h"

using namespace rma;

namespace {

struct Entry {
	int64_t	gt_off = 0, def_end = 0, first = 0, slen = 0;
	std::string	sid, sdef, letters;
};

struct Result {
	std::vector<Entry>	entries;
	int64_t	refused_at = -1;	// byte offset of the '>' of the first entry that is refused
	size_t	refused_entry = 0;
	std::string	why;
};

bool same( const FdSummary &a, const FdSummary &b )
{
	return a.letters[ 0 ] == b.letters[ 0 ] && a.letters[ 1 ] == b.letters[ 1 ] && a.starts[ 0 ] == b.starts[ 0 ] &&
		a.starts[ 1 ] == b.starts[ 1 ] && a.out == b.out;
}

// summarise -> scan (two levels, FD_SCAN_BLOCK summaries to a block) -> apply, then the host half of
// rma_db_create_device_fasta: names and refusals from the definition lines
bool run_rule( const std::string &text, int64_t chunk, int64_t lim, Result &res )
{
	const unsigned char	*t = reinterpret_cast<const unsigned char *>( text.data() );
	const int64_t	bytes = int64_t( text.size() ), chunks = ( bytes + chunk - 1 ) / chunk;
	const int64_t	blocks = ( chunks + FD_SCAN_BLOCK - 1 ) / FD_SCAN_BLOCK;
	const size_t	n_chunks = size_t( chunks ), n_blocks = size_t( blocks );
	std::vector<FdSummary>	sum( n_chunks ), local( n_chunks ), block_sum( n_blocks );
	for( int64_t c = 0; c < chunks; c++ )
		sum[ size_t( c ) ] = fd_summarise( t + c * chunk, std::min( chunk, bytes - c * chunk ) );
	for( int64_t b = 0; b < blocks; b++ ){
		FdSummary	r = fd_identity<uint32_t>();
		for( int64_t c = b * FD_SCAN_BLOCK; c < std::min<int64_t>( chunks, ( b + 1 ) * FD_SCAN_BLOCK ); c++ ){
			local[ size_t( c ) ] = r;
			r = fd_compose( r, sum[ size_t( c ) ] );
		}
		block_sum[ size_t( b ) ] = r;
	}
	std::vector<FdPrefix>	block_pre( n_blocks );
	FdPrefix	totals{ 0, 0, 0, 0 };
	for( int64_t b = 0; b < blocks; b++ ){
		block_pre[ size_t( b ) ] = totals;
		totals = fd_advance( totals, block_sum[ size_t( b ) ] );
	}
	// the whole text as one run says the same
	const FdSummary	whole = fd_summarise( t, bytes );
	if( totals.letters != whole.letters[ 0 ] || totals.starts != whole.starts[ 0 ] || totals.state != int( whole.out & 1u ) ){
		printf( "chunk %lld: the scan's totals differ from the text summarised in one run\n", ( long long )chunk );
		return false;
	}
	std::string	clean( size_t( totals.letters ), '?' );
	std::vector<Entry>	&en = res.entries;
	en.assign( size_t( totals.starts ), Entry() );
	std::vector<char>	seen_end( en.size(), 0 );
	for( int64_t c = 0; c < chunks; c++ ){
		FdPrefix	p = fd_advance( block_pre[ size_t( c / FD_SCAN_BLOCK ) ], local[ size_t( c ) ] );
		int	state = p.state;
		for( int64_t i = c * chunk; i < std::min( bytes, ( c + 1 ) * chunk ); i++ ){
			const unsigned	k = fd_apply_byte( fd_class( t[ i ] ), &state );
			if( k & FD_LETTER ){
				if( p.letters >= totals.letters ){ printf( "chunk %lld: a letter past the clean text\n", ( long long )chunk ); return false; }
				clean[ size_t( p.letters++ ) ] = char( t[ i ] );
			}else if( k & FD_GT ){
				if( p.starts >= totals.starts ){ printf( "chunk %lld: an entry past the last\n", ( long long )chunk ); return false; }
				en[ size_t( p.starts ) ].gt_off = i;
				en[ size_t( p.starts ) ].first = p.letters;
				p.starts++;
			}else if( k & FD_NL ){
				if( p.starts < 1 ){ printf( "chunk %lld: a definition line ends before any entry\n", ( long long )chunk ); return false; }
				en[ size_t( p.starts - 1 ) ].def_end = i;
				seen_end[ size_t( p.starts - 1 ) ] = 1;
			}
		}
		const FdPrefix	q = fd_advance( fd_advance( block_pre[ size_t( c / FD_SCAN_BLOCK ) ], local[ size_t( c ) ] ), sum[ size_t( c ) ] );
		if( q.letters != p.letters || q.starts != p.starts || q.state != state ){
			printf( "chunk %lld: chunk %lld's summary differs from what the pass over it finds\n", ( long long )chunk, ( long long )c );
			return false;
		}
	}
	if( totals.state == 1 && !en.empty() ){
		en.back().def_end = bytes;
		seen_end.back() = 1;
	}
	for( size_t i = 0; i < en.size(); i++ )
		if( !seen_end[ i ] ){
			printf( "chunk %lld: entry %zu's definition line has no end\n", ( long long )chunk, i );
			return false;
		}
	res.refused_at = -1;
	if( bytes > 0 && t[ 0 ] != '>' ){
		res.refused_at = 0;
		res.refused_entry = 0;
		res.why = "not >";
		return true;
	}
	for( size_t i = 0; i < en.size(); i++ ){
		Entry	&e = en[ i ];
		e.slen = ( i + 1 < en.size() ? en[ i + 1 ].first : totals.letters ) - e.first;
		e.letters = clean.substr( size_t( e.first ), size_t( e.slen ) );
		const int64_t	line = e.def_end - e.gt_off, held = std::min<int64_t>( line, FD_HEADER_CAP );
		const char	*h = text.data() + e.gt_off, *rest = nullptr;
		const int	why = line > FD_HEADER_CAP ? int( DEFLINE_LONG ) : parse_defline( h, h + held, e.sid, e.sdef, &rest );
		if( why != DEFLINE_OK || e.slen >= lim ){
			res.refused_at = e.gt_off;
			res.refused_entry = i;
			res.why = why != DEFLINE_OK ? "definition line" : "length";
			return true;
		}
		e.sid.resize( strlen( e.sid.c_str() ) );
	}
	return true;
}

// the reader's letter of a byte the rule kept (PackFile::unpack: lower case, u as t)
char reader_letter( char c )
{
	c = char( c | 0x20 );
	return c == 'u' ? 't' : c;
}

bool check_file( const char *path, int64_t lim, const std::vector<int64_t> &chunk_sizes )
{
	std::string	text;
	{
		FILE	*fp = fopen( path, "rb" );
		if( !fp ){ perror( path ); return false; }
		char	buf[ 65536 ];
		size_t	n;
		while( ( n = fread( buf, 1, sizeof( buf ), fp ) ) > 0 )
			text.append( buf, n );
		fclose( fp );
	}
	// the parallel reader: its entries up to the first it leaves to the serial reader
	std::vector<Entry>	want;
	int64_t	stopped = -1;
	std::vector<int64_t>	starts;
	{
		FastaStream	fs;
		if( !fs.open( path, int( lim ), 3 ) ){ printf( "%s: cannot be mapped\n", path ); return false; }
		int64_t	at = 0;
		for( size_t i = 0; i < fs.n_entries(); i++ ){
			starts.push_back( at );
			at += fs.extent( i );
		}
		while( std::unique_ptr<PackFile> pk = fs.next( 1000 ) )
			for( int i = 0; i < pk->count(); i++ ){
				Entry	e;
				e.sid = pk->sid( i );
				e.sdef = pk->sdef( i );
				e.slen = pk->slen[ i ];
				e.letters = pk->unpack( i );
				want.push_back( e );
			}
		stopped = fs.stopped_at();
	}
	for( int64_t chunk : chunk_sizes ){
		Result	got;
		if( !run_rule( text, chunk > 0 ? chunk : FD_CHUNK, lim, got ) ){
			printf( "%s\n", path );
			return false;
		}
		if( ( got.refused_at >= 0 ) != ( stopped >= 0 ) || ( stopped >= 0 && ( got.refused_at != stopped || got.refused_entry != want.size() ) ) ){
			printf( "%s, chunk %lld: the rule refuses at byte %lld (entry %zu), the reader hands over at byte %lld (entry %zu)\n", path,
				( long long )chunk, ( long long )got.refused_at, got.refused_entry, ( long long )stopped, want.size() );
			return false;
		}
		if( text.empty() || text[ 0 ] == '>' ){
			// the reader's cut of the file (every entry, refused or not) is the rule's
			if( starts.size() != got.entries.size() ){
				printf( "%s, chunk %lld: %zu entries, the reader finds %zu\n", path, ( long long )chunk, got.entries.size(), starts.size() );
				return false;
			}
			for( size_t i = 0; i < starts.size(); i++ ){
				const char	*nl = static_cast<const char *>( memchr( text.data() + starts[ i ], '\n', text.size() - size_t( starts[ i ] ) ) );
				const int64_t	line_end = nl ? int64_t( nl - text.data() ) : int64_t( text.size() );
				if( got.entries[ i ].gt_off != starts[ i ] || got.entries[ i ].def_end != line_end ){
					printf( "%s, chunk %lld: entry %zu at [%lld, %lld), the reader has it at [%lld, %lld)\n", path, ( long long )chunk, i,
						( long long )got.entries[ i ].gt_off, ( long long )got.entries[ i ].def_end, ( long long )starts[ i ], ( long long )line_end );
					return false;
				}
			}
		}
		const size_t	n = stopped >= 0 ? got.refused_entry : got.entries.size();
		if( n != want.size() ){
			printf( "%s, chunk %lld: %zu entries accepted, the reader delivers %zu\n", path, ( long long )chunk, n, want.size() );
			return false;
		}
		for( size_t i = 0; i < n; i++ ){
			const Entry	&g = got.entries[ i ], &w = want[ i ];
			std::string	letters = g.letters;
			for( char &c : letters )
				c = reader_letter( c );
			if( g.sid != w.sid || g.sdef != w.sdef || g.slen != w.slen || letters != w.letters ){
				printf( "%s, chunk %lld: entry %zu differs: '%s' '%s' %lld letters, the reader '%s' '%s' %lld letters\n", path, ( long long )chunk, i,
					g.sid.c_str(), g.sdef.c_str(), ( long long )g.slen, w.sid.c_str(), w.sdef.c_str(), ( long long )w.slen );
				return false;
			}
		}
	}
	return true;
}

FdSummary random_summary( std::mt19937 &rng )
{
	// summaries of random short runs, so that every one is one a text can have
	static const char	pool[] = ">\n\nAc1 >g\r";
	unsigned char	buf[ 12 ];
	const int	n = int( rng() % 12 );
	for( int i = 0; i < n; i++ )
		buf[ i ] = ( unsigned char )pool[ rng() % ( sizeof( pool ) - 1 ) ];
	return fd_summarise( buf, n );
}

}	// namespace

int main( int argc, char **argv )
{
	if( argc >= 4 && !strcmp( argv[ 1 ], "compose" ) ){
		const long	n = atol( argv[ 2 ] );
		std::mt19937	rng( unsigned( atol( argv[ 3 ] ) ) );
		for( long i = 0; i < n; i++ ){
			const FdSummary	a = random_summary( rng ), b = random_summary( rng ), c = random_summary( rng );
			if( !same( fd_compose( fd_compose( a, b ), c ), fd_compose( a, fd_compose( b, c ) ) ) ){
				printf( "triple %ld: ( a b ) c differs from a ( b c )\n", i );
				return 1;
			}
			if( !same( fd_compose( a, fd_identity<uint32_t>() ), a ) || !same( fd_compose( fd_identity<uint32_t>(), a ), a ) ){
				printf( "triple %ld: the identity is not neutral\n", i );
				return 1;
			}
		}
		printf( "%ld triples associative\n", n );
		return 0;
	}
	if( argc >= 5 && !strcmp( argv[ 1 ], "files" ) ){
		const int64_t	lim = atoll( argv[ 2 ] );
		std::vector<int64_t>	chunk_sizes;
		for( const char *p = argv[ 3 ]; *p; ){
			chunk_sizes.push_back( strtoll( p, const_cast<char **>( &p ), 10 ) );
			if( *p == ',' )
				p++;
		}
		int	n = 0;
		for( int i = 4; i < argc; i++, n++ )
			if( !check_file( argv[ i ], lim, chunk_sizes ) )
				return 1;
		printf( "%d files identical at %zu chunk sizes, FD_CHUNK %d FD_SCAN_BLOCK %d FD_HEADER_CAP %d\n", n, chunk_sizes.size(), FD_CHUNK,
			FD_SCAN_BLOCK, FD_HEADER_CAP );
		return 0;
	}
	fprintf( stderr, "usage: fasta_index_check files maxslen chunks file... | compose n seed\n" );
	return 2;
}
