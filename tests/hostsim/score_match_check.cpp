// score_match_check.cpp -- the rule of rnamotif_amd/csrc/rm_score_core.h for an image with expressions (=~, !~ and
// mismatches( string, pattern ): rms_run_t< *, true >, the matcher of rm_seqcheck.h in planes of stride 1), on the host.
//
//   score_match_check run ENTRIES RECORDS BUDGET FLAGS HEAP STRIDE DESCRIPTOR-ARGUMENTS...
// As score_text_check run, for an image opened with FLAGS (1 checked, 2 text, 8 match): "REFUSED <words>", or "IMAGE ..."
// and a line for every record,
//   A <kind> <the SCORE's double as 16 hex digits> <length> <the score column as hex digits>
//   R 0 0000000000000000 0 -
//   S 0 0000000000000000 0 - <words>
// With FLAGS & 2 the rule is rms_run_t< true, true > with a heap of HEAP bytes and, STRIDE > 0, a row for the score
// column; without, rms_run_t< false, true >.  The host side is ScoreVM::run and HitPrinter::print.  The two must agree:
// outcome, kind, bits, column; for a stop the host VM has too, its words; the budget, the heap, string + without a heap
// and the row must meet a host VM that did not fail.  "MISMATCH record ..." and status 1 otherwise.  At the end the host
// VM's side alone is counted: "VM A=<accepted> R=<rejected> S=<stopped> scores=<int SCORE>:<records>,...".
//
//   score_match_check strings PATTERN ENTRIES RECORDS BUDGET FLAGS HEAP STRIDE DESCRIPTOR-ARGUMENTS...
// The same, and every accepted record's SCORE must be 2 * n_mm + step + 1000 * ( 2 * n_mm0 + step0 ): re_step() and
// re_mm_step() of rm_regex.cpp ( l_mm = 20 * strlen( PATTERN ) ) for PATTERN over the text of the record's first element,
// and over "".  "STRINGS checked=<n> bad=<n>"; status 1 if one is bad.
#include "rm_cli.h"
#include "rm_score.h"
#include "rm_score_core.h"
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>

using namespace rma;

namespace {

std::vector<char> slurp( const char *path )
{
	std::ifstream	f( path, std::ios::binary );
	if( !f ){
		fprintf( stderr, "score_match_check: cannot read %s\n", path );
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
	const bool	strings = argc >= 3 && !strcmp( argv[ 1 ], "strings" );
	const std::string	pattern = strings ? argv[ 2 ] : "";
	if( strings ){		// (the pattern out of the way: the rest as `run`)
		argv[ 2 ] = argv[ 1 ];
		argv++;
		argc--;
	}
	if( argc < 9 || ( strcmp( argv[ 1 ], "run" ) && !strings ) ){
		fprintf( stderr, "usage: score_match_check run ENTRIES RECORDS BUDGET FLAGS HEAP STRIDE DESCRIPTOR-ARGUMENTS... | strings PATTERN ENTRIES ...\n" );
		return 2;
	}
	const std::vector<char>	eb = slurp( argv[ 2 ] ), rb = slurp( argv[ 3 ] );
	int	budget = atoi( argv[ 4 ] );
	if( budget <= 0 )
		budget = RMS_DEFAULT_BUDGET;
	const unsigned	flags = unsigned( atoi( argv[ 5 ] ) );
	const int	heap_cap = atoi( argv[ 6 ] ), row_cap = atoi( argv[ 7 ] );
	std::vector<char *>	av{ argv[ 0 ] };
	for( int i = 8; i < argc; i++ )
		av.push_back( argv[ i ] );
	Prepared	pr;
	try{
		pr = prepare( parse_args( int( av.size() ), av.data() ) );
	}catch( Error &e ){
		fprintf( stderr, "score_match_check: %s\n", e.what() );
		return 2;
	}
	Descriptor	&d = *pr.descr;
	const rma_program_t	&prog = *pr.prog;
	ScoreImage	img;
	const std::string	why = score_image_make_flags( d, prog, &img, flags );
	if( !why.empty() ){
		printf( "REFUSED %s\n", why.c_str() );
		return 0;
	}
	const RmsImage	*m = img.image();
	const int	frames = rms_frames( m );
	printf( "IMAGE inst=%d vars=%d deepest=%d stack=%d bytes=%d pool=%d pairsets=%d wave_bytes=%d flags=%d bits_L=%d table=%zu expr=%d ops=%d frames=%d\n", m->n_inst, m->n_vars,
		img.deepest, m->stack, m->bytes, m->n_pool, m->n_ps, rms_wave_bytes( m->stack, m->n_vars, frames ), m->flags, m->bits_L, img.bits_tab.size(),
		m->n_expr, frames >= 0 ? rms_match( m )->n_ops : 0, frames );

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
	char	*pbuf = nullptr;
	size_t	psize = 0;
	FILE	*pf = open_memstream( &pbuf, &psize );
	HitPrinter	printer( d, pf );

	std::vector<int32_t>	planes( size_t( m->stack + m->n_vars ) * 3 );
	std::vector<uint8_t>	estk( RMS_ESTK ), heap( size_t( heap_cap ) + 4 ), row( size_t( row_cap ) + 4 );
	RmsMem<1>	mem{ planes.data(), estk.data(), m->stack, m->n_vars };
	const bool	with_text = ( flags & 2u ) != 0;
	if( with_text ){
		mem.heap = heap.data();
		mem.heap_cap = heap_cap;
	}
	std::vector<int32_t>	mq( size_t( rmq_slots( frames < 0 ? 0 : frames ) ), 0 );
	mem.mq = mq.data();
	mem.mq_frames = frames < 0 ? 0 : frames;
	long	vm_a = 0, vm_r = 0, vm_s = 0, str_checked = 0, str_bad = 0;
	std::map<long long, long>	vm_scores;
	ReProg	str_re;
	const bool	str_ok = strings && re_compile( pattern.c_str(), str_re );
	RmsText	tx;
	tx.bits_tab = img.bits_tab.empty() ? nullptr : img.bits_tab.data();
	if( with_text && row_cap > 0 ){
		tx.row = row.data();
		tx.row_cap = row_cap;
	}
	std::string	rc;
	int	cur = -1, status = 0;
	for( int64_t h = 0; h < n; h++ ){
		const int32_t	*w = recs + h * stride;
		const int	seq = w[ 0 ], comp = w[ 1 ];
		if( seq < 0 || seq >= n_seq || ( comp != 0 && comp != 1 ) ){
			fprintf( stderr, "score_match_check: record %lld: entry %d, strand %d\n", ( long long )h, seq, comp );
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
		int	len = 0;
		for( int e = 0; e < prog.n_elems; e++ ){
			Strel	&s = d.descr[ size_t( e ) ];
			s.matchoff = w[ RMA_HIT_HDR + 4 * e ];
			s.matchlen = w[ RMA_HIT_HDR + 4 * e + 1 ];
			s.n_mispairs = w[ RMA_HIT_HDR + 4 * e + 2 ];
			s.n_mismatches = w[ RMA_HIT_HDR + 4 * e + 3 ];
			len += s.matchlen;
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
		d.lval->ival = len;
		char	vm_out = 'R';
		int	vm_kind = 0;
		uint64_t	vm_bits = 0;
		std::string	vm_words, vm_field;
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
					vm_kind = RMS_KIND_STRING;
				// the printed line: the name in 12 columns, a blank, the score column, then what follows here
				fflush( pf );
				const size_t	from = psize;
				printer.print( "e", "", comp, slen, sbuf, nullptr );
				fflush( pf );
				std::string	out( pbuf + from, psize - from );
				out.erase( 0, out.rfind( '\n', out.size() - 2 ) + 1 );		// (the line behind the header and the definition line)
				char	tail[ 64 ];
				snprintf( tail, sizeof( tail ), " %d %7d %4d ", comp, d.pval->ival, len );
				const size_t	at = out.rfind( tail );
				if( out.size() < 13 || at == std::string::npos || at < 13 ){
					fprintf( stderr, "score_match_check: record %lld: a printed line without its columns: %s", ( long long )h, out.c_str() );
					return 2;
				}
				vm_field = out.substr( 13, at - 13 );
			}
		}catch( Error &e ){
			vm_out = 'S';
			vm_words = e.what();
		}
		// ---- the rule
		RmsResult	r;
		if( with_text )
			rms_run_t<true, true>( m, w, slen, HostBases{ sbuf, slen }, mem, budget, &r, tx );
		else
			rms_run_t<false, true>( m, w, slen, HostBases{ sbuf, slen }, mem, budget, &r, RmsText() );
		// the host VM's side, counted
		if( vm_out == 'A' ){
			vm_a++;
			if( vm_kind == RMS_KIND_INT )
				vm_scores[ ( long long )d.sval->ival ]++;
		}else if( vm_out == 'R' )
			vm_r++;
		else
			vm_s++;
		if( strings ){
			const std::string	el( sbuf + w[ RMA_HIT_HDR ], size_t( w[ RMA_HIT_HDR + 1 ] ) );
			int	n_mm = 0, n_mm0 = 0, st = 0, st0 = 0;
			if( str_ok ){
				const bool	anch = pattern[ 0 ] == '^';
				const int	l_mm = 20 * int( pattern.size() );
				st = re_step( str_re, el.c_str(), anch );
				st0 = re_step( str_re, "", anch );
				re_mm_step( str_re, el.c_str(), anch, l_mm, &n_mm );
				re_mm_step( str_re, "", anch, l_mm, &n_mm0 );
			}
			const double	want = 2 * n_mm + st + 1000 * ( 2 * n_mm0 + st0 );
			str_checked++;
			if( ( r.outcome != RMS_ACCEPT || r.kind != RMS_KIND_INT || r.score != want ) && str_bad++ < 10 )
				printf( "BAD '%s' over '%s': re_step %d, re_mm_step leaves %d; over \"\": %d, %d; the rule's outcome %d, SCORE %.0f\n", pattern.c_str(), el.c_str(), st, n_mm,
					st0, n_mm0, r.outcome, r.score );
		}
		const char	out = r.outcome == RMS_ACCEPT ? 'A' : r.outcome == RMS_REJECT ? 'R' : 'S';
		const std::string	words = out == 'S' ? score_stop_text( img, r ) : "";
		const uint64_t	bits = out == 'A' ? bits_of( r.score ) : 0;
		const std::string	field = out == 'A' && tx.row != nullptr ? std::string( reinterpret_cast<char *>( row.data() ), size_t( r.text_len ) ) : "";
		std::string	hex = field.empty() ? "-" : "";
		for( unsigned char ch : field ){
			char	b[ 4 ];
			snprintf( b, sizeof( b ), "%02x", ch );
			hex += b;
		}
		printf( "%c %d %016" PRIx64 " %d %s%s%s\n", out, out == 'A' ? r.kind : 0, bits, out == 'A' ? r.text_len : 0, hex.c_str(), out == 'S' ? " " : "", words.c_str() );
		bool	same;
		if( out == 'S' )
			switch( r.stop ){
			case RMS_STOP_BUDGET : case RMS_STOP_STRCAT : case RMS_STOP_SCORE_STRING : case RMS_STOP_HEAP : case RMS_STOP_TEXT_ROOM : case RMS_STOP_TEXT_RANGE :
			case RMS_STOP_SPF_NO_ARG : case RMS_STOP_SPF_NEED_FLOAT : case RMS_STOP_SPF_NEED_INT : case RMS_STOP_SPF_NEED_STRING : case RMS_STOP_SPF_UNSUPPORTED :
			case RMS_STOP_SPF_EG : case RMS_STOP_SPF_MODIFIER : case RMS_STOP_SPF_PREC : case RMS_STOP_SPF_RANGE : case RMS_STOP_BITS_SPAN :
				same = vm_out != 'S';		// (the host VM has the room, or goes on behind a noted error)
				break;
			default :
				same = vm_out == 'S' && words == vm_words;
				break;
			}
		else
			same = out == vm_out && ( out != 'A' || ( r.kind == vm_kind && bits == ( vm_kind == RMS_KIND_STRING ? 0 : vm_bits ) && ( tx.row == nullptr || field == vm_field ) ) );
		if( !same && status == 0 ){
			printf( "MISMATCH record %lld: the VM %c %d %016" PRIx64 " [%s] %s; the rule %c %d %016" PRIx64 " [%s] %s (pc %d)\n", ( long long )h, vm_out, vm_kind,
				vm_bits, vm_field.c_str(), vm_words.c_str(), out, r.kind, bits, field.c_str(), words.c_str(), r.pc );
			status = 1;
		}
	}
	printf( "VM A=%ld R=%ld S=%ld scores=", vm_a, vm_r, vm_s );
	for( const auto &kv : vm_scores )
		printf( "%lld:%ld,", kv.first, kv.second );
	printf( "\n" );
	if( strings ){
		printf( "STRINGS checked=%ld bad=%ld\n", str_checked, str_bad );
		status |= str_bad != 0;
	}
	fclose( pf );
	free( pbuf );
	return status;
}
