// score_check.cpp -- the rule of rnamotif_amd/csrc/rm_score_core.h against ScoreVM::run, on the host.
//
//   score_check ENTRIES RECORDS BUDGET DESCRIPTOR-ARGUMENTS...
//
// ENTRIES: int32 n, int32 len[ n ], then the entries' letters as the readers deliver them; RECORDS: int32 hit records of
// the descriptor's stride; BUDGET: instructions per record, 0 for the default.  The descriptor is compiled by the host
// front end and its image opened (rm_score_image.cpp).  A refusal prints "REFUSED <words>" and ends with status 0.
// Otherwise "IMAGE ..." with the image's sizes, then for every record both sides run -- ScoreVM::run on the descriptor
// with the record restored into it as Replayer::one_hit restores it, BEGIN run before the first, and rms_run() on the
// image over planes of stride 1 -- and one line is printed:
//   A <kind> <the SCORE's double as 16 hex digits>     accepted
//   R 0 0000000000000000                               rejected
//   S 0 0000000000000000 <words>                       stopped, with the rule's words
// The two sides must agree: the same outcome; for an accepted record the same kind of SCORE and the same bits; for a
// stopped one the words of the host VM's fail().  The first disagreement is printed as "MISMATCH record ..." and the
// status is 1.  A stop by the budget has no counterpart: the host VM must then not have failed.
#include "rm_cli.h"
#include "rm_score.h"
#include "rm_score_core.h"
#include <cinttypes>
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
		fprintf( stderr, "score_check: cannot read %s\n", path );
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

struct HostBases {
	const char	*s;
	int	slen;
	unsigned char	operator()( int i ) const { return unsigned( i ) < unsigned( slen ) ? static_cast<unsigned char>( s[ i ] ) : 'n'; }
};

uint64_t bits_of( double d )
{
	uint64_t	u;
	memcpy( &u, &d, sizeof( u ) );
	return u;
}

}	// namespace

int main( int argc, char **argv )
{
	if( argc < 5 ){
		fprintf( stderr, "usage: score_check ENTRIES RECORDS BUDGET DESCRIPTOR-ARGUMENTS...\n" );
		return 2;
	}
	const std::vector<char>	eb = slurp( argv[ 1 ] ), rb = slurp( argv[ 2 ] );
	int	budget = atoi( argv[ 3 ] );
	if( budget <= 0 )
		budget = RMS_DEFAULT_BUDGET;
	std::vector<char *>	av{ argv[ 0 ] };
	for( int i = 4; i < argc; i++ )
		av.push_back( argv[ i ] );
	Prepared	pr;
	try{
		pr = prepare( parse_args( int( av.size() ), av.data() ) );
	}catch( Error &e ){
		fprintf( stderr, "score_check: %s\n", e.what() );
		return 2;
	}
	Descriptor	&d = *pr.descr;
	const rma_program_t	&prog = *pr.prog;
	ScoreImage	img;
	const std::string	why = score_image_make( d, prog, &img );
	if( !why.empty() ){
		printf( "REFUSED %s\n", why.c_str() );
		return 0;
	}
	const RmsImage	*m = img.image();
	printf( "IMAGE inst=%d vars=%d deepest=%d stack=%d bytes=%d pool=%d pairsets=%d wave_bytes=%d\n", m->n_inst, m->n_vars, img.deepest, m->stack,
		m->bytes, m->n_pool, m->n_ps, rms_wave_bytes( m->stack, m->n_vars ) );

	const int32_t	*ew = reinterpret_cast<const int32_t *>( eb.data() );
	const int	n_seq = eb.size() >= 4 ? ew[ 0 ] : 0;
	std::vector<const char *>	text( static_cast<size_t>( n_seq ), nullptr );
	const char	*tp = eb.data() + 4 * ( size_t( n_seq ) + 1 );
	for( int i = 0; i < n_seq; i++ ){
		text[ size_t( i ) ] = tp;
		tp += ew[ 1 + i ];
	}
	const int	stride = rma_hit_stride( &prog ), ctx_off = rma_hit_ctx_off( &prog ), efn_off = rma_hit_efn_off( &prog );
	const int64_t	n = int64_t( rb.size() / 4 / size_t( stride ) );
	const int32_t	*recs = reinterpret_cast<const int32_t *>( rb.data() );

	// Replayer::begin()
	d.score->setprog( P_BEGIN );
	d.score->run( 0, 0, nullptr, nullptr, nullptr );
	d.score->setprog( P_MAIN );

	std::vector<int32_t>	planes( size_t( m->stack + m->n_vars ) * 3 );
	std::vector<uint8_t>	estk( RMS_ESTK );
	const RmsMem<1>	mem{ planes.data(), estk.data(), m->stack, m->n_vars };
	std::string	rc;
	int	cur = -1, status = 0;
	for( int64_t h = 0; h < n; h++ ){
		const int32_t	*w = recs + h * stride;
		const int	seq = w[ 0 ], comp = w[ 1 ];
		if( seq < 0 || seq >= n_seq || ( comp != 0 && comp != 1 ) ){
			fprintf( stderr, "score_check: record %lld: entry %d, strand %d\n", ( long long )h, seq, comp );
			return 2;
		}
		const int	slen = ew[ 1 + seq ];
		if( comp && seq != cur ){
			rc.assign( size_t( slen ), 'n' );
			for( int i = 0; i < slen; i++ )
				rc[ size_t( slen - 1 - i ) ] = wc_cmp( text[ size_t( seq ) ][ i ] );
			cur = seq;
		}
		std::string	fwd;
		const char	*sbuf;
		if( comp )
			sbuf = rc.c_str();
		else{
			fwd.assign( text[ size_t( seq ) ], size_t( slen ) );		// (the VM's strings end with a NUL)
			sbuf = fwd.c_str();
		}
		// ---- the host VM, the record restored as Replayer::one_hit restores it
		for( int e = 0; e < prog.n_elems; e++ ){
			Strel	&s = d.descr[ size_t( e ) ];
			s.matchoff = w[ RMA_HIT_HDR + 4 * e ];
			s.matchlen = w[ RMA_HIT_HDR + 4 * e + 1 ];
			s.n_mispairs = w[ RMA_HIT_HDR + 4 * e + 2 ];
			s.n_mismatches = w[ RMA_HIT_HDR + 4 * e + 3 ];
		}
		if( d.lctx ){
			d.lctx->matchoff = w[ ctx_off ];
			d.lctx->matchlen = w[ ctx_off + 1 ];
		}
		if( d.rctx ){
			d.rctx->matchoff = w[ ctx_off + 2 ];
			d.rctx->matchlen = w[ ctx_off + 3 ];
		}
		d.nval->pval = const_cast<char *>( "e" );
		d.cval->ival = comp;
		d.pval->ival = comp ? slen - d.descr[ 0 ].matchoff : d.descr[ 0 ].matchoff + 1;
		int	len = 0;
		for( int e = 0; e < prog.n_elems; e++ )
			len += d.descr[ size_t( e ) ].matchlen;
		d.lval->ival = len;
		char	vm_out = 'R';
		int	vm_kind = 0;
		uint64_t	vm_bits = 0;
		std::string	vm_words;
		try{
			Ident	*h_id = nullptr;
			if( d.score->run( comp, slen, sbuf, &h_id, prog.n_efn_sites ? w + efn_off : nullptr ) != SA_REJECT ){
				vm_out = 'A';
				const Value	*sv = d.sval;
				if( sv->type == T_INT ){
					vm_kind = RMS_KIND_INT;
					vm_bits = bits_of( double( sv->ival ) );
				}else if( sv->type == T_FLOAT ){
					vm_kind = RMS_KIND_FLOAT;
					vm_bits = bits_of( sv->dval );
				}else if( sv->type == T_STRING )
					vm_kind = 3;
			}
		}catch( Error &e ){
			vm_out = 'S';
			vm_words = e.what();
		}
		// ---- the rule
		RmsResult	r;
		rms_run( m, w, slen, HostBases{ sbuf, slen }, mem, budget, &r );
		const char	out = r.outcome == RMS_ACCEPT ? 'A' : r.outcome == RMS_REJECT ? 'R' : 'S';
		const std::string	words = out == 'S' ? score_stop_text( img, r ) : "";
		const uint64_t	bits = out == 'A' ? bits_of( r.score ) : 0;
		printf( "%c %d %016" PRIx64 "%s%s\n", out, out == 'A' ? r.kind : 0, bits, out == 'S' ? " " : "", words.c_str() );
		bool	same;
		if( out == 'S' && r.stop == RMS_STOP_BUDGET )
			same = vm_out != 'S';
		else if( out == 'S' && ( r.stop == RMS_STOP_STRCAT || r.stop == RMS_STOP_SCORE_STRING ) )
			same = vm_out != 'S';		// (the host VM has the buffer, and prints a string)
		else
			same = out == vm_out && ( out != 'A' || ( r.kind == vm_kind && bits == vm_bits ) ) && ( out != 'S' || words == vm_words );
		if( !same && status == 0 ){
			printf( "MISMATCH record %lld: the VM %c %d %016" PRIx64 " %s; the rule %c %d %016" PRIx64 " %s (pc %d)\n", ( long long )h, vm_out, vm_kind,
				vm_bits, vm_words.c_str(), out, r.kind, bits, words.c_str(), r.pc );
			status = 1;
		}
	}
	return status;
}
