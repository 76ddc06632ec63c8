// seq_check.cpp -- the rule of rnamotif_amd/csrc/rm_seqcheck.h against re_step() / re_mm_step() of rm_regex.cpp, on the host.
//
//   seq_check ENTRIES RECORDS BUDGET DESCRIPTOR-ARGUMENTS...
//
// ENTRIES: int32 n, int32 len[ n ], then the entries' letters as the readers deliver them; RECORDS: int32 hit records of
// the descriptor's stride; BUDGET: ops per record, 0 for the default.  The descriptor is compiled by the host front end
// and the image of its loose seq= expressions made (rm_seqcheck.cpp).  A refusal prints "REFUSED <words>" and ends with
// status 0.  Otherwise "IMAGE ..." with the image's sizes, then for every record both sides run -- the loose elements as
// Replayer::one_hit applies them, a NUL terminated copy of the element's text through the recursive matcher, and
// rmq_run() on the image over planes of stride 1, reading the strand through an accessor -- and one line is printed:
//   K -1 <steps> <the fixed row's words>        kept
//   D <element> <steps> <the fixed row's words>  dropped at this element
//   S <element> <steps> <the fixed row's words>  stopped at this element: more than BUDGET steps
// The two sides must agree: the same outcome at the same element, and for a kept record the mismatch words one_hit
// leaves in the elements.  The first disagreement is printed as "MISMATCH record ..." and the status is 1.  A stop by
// the budget has no counterpart on the other side.
#include "rm_cli.h"
#include "rm_regex.h"
#include "rm_seqcheck.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

using namespace rma;

namespace {

std::vector<char> slurp( const char *path )
{
	std::ifstream	f( path, std::ios::binary );
	if( !f ){
		fprintf( stderr, "seq_check: cannot read %s\n", path );
		exit( 2 );
	}
	return std::vector<char>( std::istreambuf_iterator<char>( f ), std::istreambuf_iterator<char>() );
}

char wc_cmp( char c )		// mk_rcmp, rnamot.c:193-216
{
	switch( c ){
	case 'a' : case 'A' : return 't';
	case 'c' : case 'C' : return 'g';
	case 'g' : case 'G' : return 'c';
	case 't' : case 'T' : case 'u' : case 'U' : return 'a';
	default : return 'n';
	}
}

// the strand, and nothing else: a read outside it ends the program
struct HostBases {
	const char	*s;
	int	slen;
	unsigned char	operator()( int i ) const
	{
		if( unsigned( i ) >= unsigned( slen ) ){
			fprintf( stderr, "seq_check: the rule read position %d of a strand of %d bases\n", i, slen );
			abort();
		}
		return static_cast<unsigned char>( s[ i ] );
	}
};

}	// namespace

int main( int argc, char **argv )
{
	if( argc < 5 ){
		fprintf( stderr, "usage: seq_check ENTRIES RECORDS BUDGET DESCRIPTOR-ARGUMENTS...\n" );
		return 2;
	}
	const std::vector<char>	eb = slurp( argv[ 1 ] ), rb = slurp( argv[ 2 ] );
	int	budget = atoi( argv[ 3 ] );
	if( budget <= 0 )
		budget = RMQ_DEFAULT_BUDGET;
	std::vector<char *>	av{ argv[ 0 ] };
	for( int i = 4; i < argc; i++ )
		av.push_back( argv[ i ] );
	Prepared	pr;
	try{
		pr = prepare( parse_args( int( av.size() ), av.data() ) );
	}catch( Error &e ){
		printf( "REFUSED compile: %s\n", e.what() );
		return 0;
	}
	Descriptor	&d = *pr.descr;
	const rma_program_t	&prog = *pr.prog;
	SeqImage	img;
	const std::string	why = seqcheck_image_make( d, prog, &img );
	if( !why.empty() ){
		printf( "REFUSED %s\n", why.c_str() );
		return 0;
	}
	const RmqImage	*m = img.image();
	printf( "IMAGE expr=%d ops=%d frames=%d bytes=%d wave_bytes=%d\n", m->n_expr, m->n_ops, m->frames, m->bytes, rmq_wave_bytes( m->frames ) );

	const int32_t	*ew = reinterpret_cast<const int32_t *>( eb.data() );
	const int	n_seq = eb.size() >= 4 ? ew[ 0 ] : 0;
	std::vector<const char *>	text( static_cast<size_t>( n_seq ), nullptr );
	const char	*tp = eb.data() + 4 * ( size_t( n_seq ) + 1 );
	for( int i = 0; i < n_seq; i++ ){
		text[ size_t( i ) ] = tp;
		tp += ew[ 1 + i ];
	}
	const int	stride = rma_hit_stride( &prog );
	const int64_t	n = int64_t( rb.size() / 4 / size_t( stride ) );
	const int32_t	*recs = reinterpret_cast<const int32_t *>( rb.data() );

	std::vector<int32_t>	planes( size_t( rmq_slots( m->frames ) ) ), fixed( static_cast<size_t>( stride ) );
	const RmqMem<1>	mem{ planes.data(), m->frames };
	std::string	rc, chk;
	int	cur = -1, status = 0;
	for( int64_t h = 0; h < n; h++ ){
		const int32_t	*w = recs + h * stride;
		const int	seq = w[ 0 ], comp = w[ 1 ];
		if( seq < 0 || seq >= n_seq || ( comp != 0 && comp != 1 ) ){
			fprintf( stderr, "seq_check: record %lld: entry %d, strand %d\n", ( long long )h, seq, comp );
			return 2;
		}
		const int	slen = ew[ 1 + seq ];
		for( int e = 0; e < prog.n_elems; e++ ){
			const int64_t	off = w[ RMA_HIT_HDR + 4 * e ], len = w[ RMA_HIT_HDR + 4 * e + 1 ];
			if( off < 0 || len < 0 || off + len > slen ){
				fprintf( stderr, "seq_check: record %lld: element %d outside its entry\n", ( long long )h, e );
				return 2;
			}
		}
		if( comp && seq != cur ){
			rc.assign( size_t( slen ), 'n' );
			for( int i = 0; i < slen; i++ )
				rc[ size_t( slen - 1 - i ) ] = wc_cmp( text[ size_t( seq ) ][ i ] );
			cur = seq;
		}
		const char	*sbuf = comp ? rc.data() : text[ size_t( seq ) ];
		// ---- Replayer::one_hit's loop over the loose elements
		char	host_out = 'K';
		int	host_elem = -1;
		std::vector<int32_t>	host_row( w, w + stride );
		for( int e = 0; e < prog.n_elems; e++ ){
			const int	ri = prog.elems[ e ].re;
			if( ri < 0 || !prog.regexes[ ri ].loose )
				continue;
			const Strel	&s = d.descr[ size_t( e ) ];
			chk.assign( sbuf + w[ RMA_HIT_HDR + 4 * e ], size_t( w[ RMA_HIT_HDR + 4 * e + 1 ] ) );
			bool	ok;
			if( s.mismatch > 0 ){
				int	n_mm = 0;
				ok = re_mm_step( *s.re, chk.c_str(), *s.seq == '^', s.mismatch, &n_mm );
				host_row[ size_t( RMA_HIT_HDR + 4 * e + 3 ) ] = n_mm;
			}else
				ok = re_step( *s.re, chk.c_str(), *s.seq == '^' );
			if( !ok ){
				host_out = 'D';
				host_elem = e;
				host_row.assign( w, w + stride );
				break;
			}
		}
		// ---- the rule
		RmqResult	r;
		memcpy( fixed.data(), w, size_t( stride ) * 4 );
		rmq_run( m, w, HostBases{ sbuf, slen }, mem, budget, fixed.data(), &r );
		const char	out = r.outcome == RMQ_KEEP ? 'K' : r.outcome == RMQ_DROP ? 'D' : 'S';
		printf( "%c %d %d", out, r.elem, r.steps );
		for( int k = 0; k < stride; k++ )
			printf( " %d", fixed[ size_t( k ) ] );
		printf( "\n" );
		const bool	same = out == 'S' ? memcmp( fixed.data(), w, size_t( stride ) * 4 ) == 0 :
			out == host_out && r.elem == host_elem && fixed == host_row;
		if( !same && status == 0 ){
			printf( "MISMATCH record %lld: the matcher %c at element %d; the rule %c at element %d after %d steps\n", ( long long )h, host_out, host_elem,
				out, r.elem, r.steps );
			status = 1;
		}
	}
	return status;
}
