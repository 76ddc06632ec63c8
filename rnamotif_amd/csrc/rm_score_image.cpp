// rm_score_image.cpp -- see rm_score_image.h: MAIN of a compiled descriptor as an image for the rule of rm_score_core.h,
// what is refused, and the host VM's words for a stop.
#include "rm_score.h"
#include "rm_score_core.h"
#include "rm_regex.h"
#include <atomic>
#include <cstdarg>
#include <cmath>
#include <cstring>
#include <map>

namespace rma {

static_assert( int( RMS_T_UNDEF ) == T_UNDEF && int( RMS_T_INT ) == T_INT && int( RMS_T_FLOAT ) == T_FLOAT && int( RMS_T_STRING ) == T_STRING &&
	int( RMS_T_PAIRSET ) == T_PAIRSET && int( RMS_T_POS ) == T_POS && int( RMS_T_IDENT ) == T_IDENT && int( RMS_T_HIT ) == T_HIT, "the rule's value types are T_*" );
static_assert( int( RMS_N_OP ) == N_OP && int( RMS_OP_SCL ) == OP_SCL && int( RMS_OP_STO ) == OP_STO && int( RMS_OP_INS ) == OP_INS &&
	int( RMS_OP_LES ) == OP_LES && int( RMS_OP_MOD ) == OP_MOD && int( RMS_OP_MM_I ) == OP_MM_I && int( RMS_OP_JMP ) == OP_JMP, "the rule's op codes are OP_*" );
static_assert( int( RMS_N_SC ) == N_SC && int( RMS_SC_EFN2 ) == SC_EFN2 && int( RMS_SC_MISMATCHES_2 ) == SC_MISMATCHES_2 &&
	int( RMS_SC_PAIRED ) == SC_PAIRED && int( RMS_SC_SUBSTR ) == SC_SUBSTR, "the rule's builtins are SC_*" );

namespace {

std::string fmt( const char *f, ... ) __attribute__(( format( printf, 1, 2 ) ));
std::string fmt( const char *f, ... )
{
	char	buf[ 1024 ];
	va_list	ap;
	va_start( ap, f );
	vsnprintf( buf, sizeof( buf ), f, ap );
	va_end( ap );
	return buf;
}

struct Builder {
	std::string	pool;
	std::vector<RmsInst>	inst;
	std::vector<double>	dbl;
	std::vector<RmsVar>	vars;
	std::vector<const Ident *>	idents;
	std::vector<rma_pairset_t>	ps;
	std::vector<const PairSet *>	ps_of;

	int	string_at( const char *s, size_t n )
	{
		const size_t	at = pool.find( std::string( s, n ) );
		if( at != std::string::npos && n > 0 )
			return int( at );
		pool.append( s, n );
		return int( pool.size() - n );
	}
	int	pairset( const PairSet *p )
	{
		for( size_t i = 0; i < ps_of.size(); i++ )
			if( ps_of[ i ] == p )
				return int( i );
		ps_of.push_back( p );
		ps.push_back( p->mat );
		return int( ps.size() ) - 1;
	}
	// the variable of an identifier, entered with what it holds now; "" or why it cannot be held
	std::string	variable( const Ident *idp, int *v )
	{
		for( size_t i = 0; i < idents.size(); i++ )
			if( idents[ i ] == idp ){
				*v = int( i );
				return "";
			}
		RmsVar	var{ idp->type, 0, 0 };
		if( idp->type == T_INT )
			var.lo = idp->val.ival;
		else if( idp->type == T_FLOAT ){
			uint64_t	u;
			memcpy( &u, &idp->val.dval, sizeof( u ) );
			var.lo = int32_t( uint32_t( u ) );
			var.hi = int32_t( uint32_t( u >> 32 ) );
		}else if( idp->type == T_STRING ){
			const char	*s = static_cast<const char *>( idp->val.pval );
			if( s == nullptr )
				return "the string variable '" + idp->name + "' holds no string";
			var.hi = int32_t( strlen( s ) );
			var.lo = string_at( s, size_t( var.hi ) );
		}
		*v = int( idents.size() );
		idents.push_back( idp );
		vars.push_back( var );
		return "";
	}
};

}	// namespace

std::string score_image_make( const Descriptor &d, const rma_program_t &prog, ScoreImage *out, bool checked )
{
	return score_image_make_flags( d, prog, out, checked ? 1u : 0u );
}

std::string score_image_make_flags( const Descriptor &d, const rma_program_t &prog, ScoreImage *out, unsigned flags )
{
	const bool	checked = ( flags & 1u ) != 0, text = ( flags & 2u ) != 0, match = ( flags & 8u ) != 0;
	static std::atomic<uint64_t>	serials{ 0 };
	const char	*who = "the score section cannot run on the device: ";
	for( int e = 0; e < prog.n_elems && !checked; e++ )
		if( prog.elems[ e ].re >= 0 && prog.regexes[ prog.elems[ e ].re ].loose )
			return std::string( who ) + fmt( "the descriptor is loose (element %d's seq= is tested by a necessary condition only): its records are "
				"not yet the reference's candidates", e );
	std::unique_ptr<Descriptor>	c;
	try{
		c = compile_descriptor( d.args, &d.expanded );
		ScoreVM	&vm = *c->score;
		vm.linkscore();
		c->stderr_text.clear();
		vm.setprog( P_BEGIN );
		vm.run( 0, 0, nullptr, nullptr, nullptr );
		vm.setprog( P_MAIN );
	}catch( Error &e ){
		return std::string( who ) + e.what();
	}
	const ScoreVM	&vm = *c->score;
	std::string	why;
	int	deepest = 0;
	if( !vm.hit_independent( &why, &deepest ) )
		return std::string( who ) + "MAIN is not independent from hit to hit: " + why;
	const std::vector<Inst>	&pr = vm.program( P_MAIN );
	const int	n_elems = int( c->descr.size() );
	if( n_elems != prog.n_elems || int( vm.efn_calls().size() ) != prog.n_efn_sites )
		return std::string( who ) + "the program is not this descriptor's";
	if( pr.size() > size_t( RMS_MAX_INST ) )
		return std::string( who ) + fmt( "MAIN has %zu instructions, the image holds %d", pr.size(), int( RMS_MAX_INST ) );

	Builder	b;
	ScoreImage	&img = *out;
	img = ScoreImage();
	img.wdfname = c->wdfname;
	img.deepest = deepest;
	// SCORE first, whether MAIN names it or not: the printer reads it
	const Ident	*score_id = nullptr, *slen_id = c->find_id( "SLEN" );
	for( auto &g : c->globals )
		if( &g.second->val == c->sval )
			score_id = g.second;
	int	v = 0;
	if( score_id == nullptr || !( why = b.variable( score_id, &v ) ).empty() )
		return std::string( who ) + ( score_id == nullptr ? "no SCORE" : why );
	std::map<std::string, int>	file_ix;
	std::vector<size_t>	marks;		// the MRK of every call and `in` that is open
	// RMA_SCORE_MATCH: the expressions of =~ / !~ and mismatches( string, pattern ), compiled here once for all records
	std::vector<RmsMatchExpr>	exprs;
	std::vector<RmqOp>	ops;
	int	frames = 0;
	std::vector<char>	landed( pr.size() + 1, 0 );	// a jump of MAIN lands on this instruction
	for( const Inst &ip : pr )
		if( ( ip.op == OP_FJP || ip.op == OP_JMP || ip.op == OP_AND || ip.op == OP_IOR ) && ip.val.ival >= 0 && size_t( ip.val.ival ) <= pr.size() )
			landed[ size_t( ip.val.ival ) ] = 1;
	// The pattern of the MAT or the SCL at pc as an expression of the table; *x: its index.  The pattern is a constant
	// where the instruction that leaves it on the stack is an LDC of a string directly in front and no jump lands between
	// the two; one a record makes would have to be compiled for every record.
	auto expression = [&]( size_t pc, const char *what, int *x ) -> std::string {
		if( pc == 0 || pr[ pc - 1 ].op != OP_LDC || pr[ pc - 1 ].val.type != T_STRING || landed[ pc ] )
			return fmt( "the pattern of %s is not one string constant: it would have to be compiled for every record", what );
		const char	*pat = static_cast<const char *>( pr[ pc - 1 ].val.pval );
		if( exprs.size() >= size_t( RMS_MAX_EXPR ) )
			return fmt( "more than %d patterns of =~, !~ and mismatches( string, pattern ), the image holds %d expressions", int( RMS_MAX_EXPR ), int( RMS_MAX_EXPR ) );
		RmsMatchExpr	ex{ *pat == '^', int32_t( ops.size() ), -1, int32_t( strlen( pat ) ) };
		ReProg	re;
		if( re_compile( pat, re ) ){
			if( re.ops.size() > size_t( RMQ_MAX_OPS ) )
				return fmt( "the pattern '%s' of %s has %zu ops, the image holds %d an expression", pat, what, re.ops.size(), int( RMQ_MAX_OPS ) );
			int	repeats = 0;
			if( !rmq_flatten( re, &ops, &repeats ) )
				return fmt( "the pattern '%s' of %s has a group number beyond 9", pat, what );
			ex.n_ops = int32_t( re.ops.size() );
			frames = std::max( frames, repeats );
		}else if( re.err != 41 )	// ("" is no expression at all -- regerr 41, no remembered search string: the host VM answers 0, and so does the rule)
			return fmt( "the pattern '%s' of %s is no regular expression (regerr %d)", pat, what, re.err );
		*x = int( exprs.size() );
		exprs.push_back( ex );
		return "";
	};
	for( size_t pc = 0; pc < pr.size(); pc++ ){
		const Inst	&ip = pr[ pc ];
		const std::string	at = fmt( "%s:%d ", ip.filename, ip.lineno );
		RmsInst	o{ uint8_t( ip.op ), RMS_K_NONE, 0, 0 };
		switch( ip.op ){
		case OP_MAT : {
			if( !match )
				return std::string( who ) + at + "the =~ and !~ operators need the host's regular expressions";
			int	x = 0;
			if( !( why = expression( pc, "=~ / !~", &x ) ).empty() )
				return std::string( who ) + at + why;
			o.kind = RMS_K_INT;
			o.a = x;
			break;
		}
		case OP_HOLD : case OP_RLSE : case OP_FCL : case OP_HALT :
			return std::string( who ) + at + "an instruction MAIN cannot hold";
		case OP_MRK :
			marks.push_back( pc );
			break;
		case OP_INS :
			if( !marks.empty() )
				marks.pop_back();
			break;
		case OP_SCL : {
			o.kind = RMS_K_INT;
			o.a = ip.val.ival;
			const size_t	mark = marks.empty() ? pr.size() : marks.back();
			if( !marks.empty() )
				marks.pop_back();
			// a format that is a constant of the pool: the first argument is one LDC, the next instruction pushes or calls
			if( o.a == SC_SPRINTF && text && mark + 2 <= pc && pr[ mark + 1 ].op == OP_LDC && pr[ mark + 1 ].val.type == T_STRING &&
				( mark + 2 == pc || pr[ mark + 2 ].op == OP_LDC || pr[ mark + 2 ].op == OP_LOD || pr[ mark + 2 ].op == OP_LDA || pr[ mark + 2 ].op == OP_MRK ) ){
				const char	*f = static_cast<const char *>( pr[ mark + 1 ].val.pval );
				for( const char *pp = f; ( pp = strchr( pp, '%' ) ) != nullptr; ){
					const char	*epp = strpbrk( pp + 1, "bBdiouxXfeEgGcCsSpn%" );
					if( epp == nullptr )
						break;
					if( strchr( "eEgG", *epp ) != nullptr )
						return std::string( who ) + at + fmt( "sprintf(): the format '%s' holds %%%c, whose digits the host's C library chooses", f, *epp );
					pp = epp + 1;
				}
			}
			if( o.a == SC_SPRINTF && !text )
				return std::string( who ) + at + "sprintf() formats text, which the host does";
			if( o.a == SC_BITS && !text )
				return std::string( who ) + at + "bits() is computed on the host";
			if( o.a == SC_MISMATCHES_2 ){
				if( !match )
					return std::string( who ) + at + "mismatches( string, pattern ) needs the host's regular expressions";
				int	x = 0;
				if( !( why = expression( pc, "mismatches( string, pattern )", &x ) ).empty() )
					return std::string( who ) + at + why;
				o.len = uint16_t( x );
			}
			if( o.a < 0 || o.a >= N_SC || o.a == SC_MISMATCHES )
				return std::string( who ) + at + "an unknown builtin";
			break;
		}
		case OP_LDA :
		case OP_LOD : {
			const Ident	*idp = static_cast<const Ident *>( ip.val.pval );
			if( &idp->val == c->nval )
				return std::string( who ) + at + "MAIN reads NAME, a string the host has";
			if( !( why = b.variable( idp, &v ) ).empty() )
				return std::string( who ) + at + why;
			o.kind = RMS_K_IDENT;
			o.a = v;
			break;
		}
		case OP_LDC :
			switch( ip.val.type ){
			case T_INT :
				o.kind = RMS_K_INT;
				o.a = ip.val.ival;
				break;
			case T_FLOAT :
				o.kind = RMS_K_FLOAT;
				o.a = int32_t( b.dbl.size() );
				b.dbl.push_back( ip.val.dval );
				break;
			case T_STRING : {
				const char	*s = static_cast<const char *>( ip.val.pval );
				const size_t	n = strlen( s );
				if( n > 0xffff )
					return std::string( who ) + at + "a string constant of more than 65535 bytes";
				o.kind = RMS_K_STRING;
				o.len = uint16_t( n );
				o.a = b.string_at( s, n );
				break;
			}
			case T_POS :
				o.kind = RMS_K_POS;
				break;
			case T_PAIRSET :
				o.kind = RMS_K_PAIRSET;
				o.a = b.pairset( static_cast<const PairSet *>( ip.val.pval ) );
				break;
			default :
				break;		// (the rule stops with the VM's "type mismatch")
			}
			break;
		case OP_FJP : case OP_JMP : case OP_AND : case OP_IOR :
			o.kind = RMS_K_INT;
			o.a = ip.val.ival;
			if( o.a < 0 || o.a >= int( pr.size() ) )
				return std::string( who ) + at + "a jump out of the program";
			break;
		default :
			break;
		}
		b.inst.push_back( o );
		auto f = file_ix.find( ip.filename );
		if( f == file_ix.end() ){
			f = file_ix.emplace( ip.filename, int( img.files.size() ) ).first;
			img.files.push_back( ip.filename );
		}
		img.file_of.push_back( f->second );
		img.line_of.push_back( ip.lineno );
	}
	// the element table: rm_descr[], the left context, the right context
	std::vector<RmsElem>	rows( size_t( n_elems ) + 2 );
	auto row_of = [&]( const Strel *s ) -> int {
		if( s == c->lctx )
			return n_elems;
		if( s == c->rctx )
			return n_elems + 1;
		return int( s - c->descr.data() );
	};
	for( int r = 0; r < n_elems + 2; r++ ){
		const Strel	*s = r < n_elems ? &c->descr[ size_t( r ) ] : r == n_elems ? c->lctx : c->rctx;
		RmsElem	&o = rows[ size_t( r ) ];
		o = RmsElem{ -1, -1, 0, -1, 0, { 0, 0, 0 }, -1 };
		if( s == nullptr )
			continue;
		o.type = s->type;
		o.index = s->index;
		if( s->tag != nullptr ){
			o.tag_len = int32_t( strlen( s->tag ) );
			o.tag_off = b.string_at( s->tag, size_t( o.tag_len ) );
		}
		o.n_mates = int32_t( s->mates.size() );
		for( int k = 0; k < 3 && k < o.n_mates; k++ ){
			o.mates[ k ] = row_of( s->mates[ size_t( k ) ] );
			if( o.mates[ k ] < 0 || o.mates[ k ] >= n_elems + 2 )
				return std::string( who ) + "an element's mate outside the descriptor";
		}
		if( o.n_mates > 0 && s->pairset != nullptr )
			o.ps = b.pairset( s->pairset );
	}
	std::vector<int32_t>	xd;
	for( const Strel *s : vm.xdescr )
		xd.push_back( row_of( s ) );
	std::vector<rma_efn_site_t>	sites;
	for( const EfnCall &ec : vm.efn_calls() )
		sites.push_back( ec.site );

	const int	stack = deepest + RMS_STACK_MARGIN;
	if( stack > RMS_MAX_STACK )
		return std::string( who ) + fmt( "MAIN's operand stack can reach %d slots, the image allows %d", deepest, RMS_MAX_STACK - RMS_STACK_MARGIN );
	if( b.vars.size() > size_t( RMS_MAX_VARS ) )
		return std::string( who ) + fmt( "MAIN names %zu variables, the image holds %d", b.vars.size(), int( RMS_MAX_VARS ) );
	if( b.ps.size() > size_t( RMS_MAX_PS ) )
		return std::string( who ) + fmt( "%zu pair sets, the image holds %d", b.ps.size(), int( RMS_MAX_PS ) );
	if( b.pool.size() > size_t( RMS_MAX_POOL ) )
		return std::string( who ) + fmt( "%zu bytes of strings, the image holds %d", b.pool.size(), int( RMS_MAX_POOL ) );

	RmsImage	h;
	memset( &h, 0, sizeof( h ) );
	h.magic = RMS_MAGIC;
	h.n_inst = int32_t( b.inst.size() );
	h.n_dbl = int32_t( b.dbl.size() );
	h.n_vars = int32_t( b.vars.size() );
	h.n_xd = int32_t( xd.size() );
	h.n_elems = n_elems;
	h.n_rows = n_elems + 2;
	h.n_ps = int32_t( b.ps.size() );
	h.n_efn = int32_t( sites.size() );
	h.n_pool = int32_t( b.pool.size() );
	h.stack = stack;
	h.x_off = c->lctx != nullptr && c->lctx_explicit ? 1 : 0;
	h.ctx_off = rma_hit_ctx_off( &prog );
	h.efn_off = rma_hit_efn_off( &prog );
	h.stride = rma_hit_stride( &prog );
	h.sym_se = SYM_SE;
	h.sym_ss = SYM_SS;
	h.v_score = 0;
	h.v_comp = h.v_pos = h.v_len = h.v_slen = -1;
	for( size_t i = 0; i < b.idents.size(); i++ ){
		const Value	*val = &b.idents[ i ]->val;
		if( val == c->cval ) h.v_comp = int32_t( i );
		if( val == c->pval ) h.v_pos = int32_t( i );
		if( val == c->lval ) h.v_len = int32_t( i );
		if( b.idents[ i ] == slen_id ) h.v_slen = int32_t( i );
		img.var_names.push_back( b.idents[ i ]->name );
	}
	size_t	at = ( sizeof( RmsImage ) + 7 ) & ~size_t( 7 );
	auto place = [&]( int32_t *o, size_t bytes ){
		*o = int32_t( at );
		at = ( at + bytes + 7 ) & ~size_t( 7 );
	};
	place( &h.o_dbl, b.dbl.size() * sizeof( double ) );
	place( &h.o_inst, b.inst.size() * sizeof( RmsInst ) );
	place( &h.o_vars, b.vars.size() * sizeof( RmsVar ) );
	place( &h.o_xd, xd.size() * sizeof( int32_t ) );
	place( &h.o_rows, rows.size() * sizeof( RmsElem ) );
	place( &h.o_ps, b.ps.size() * sizeof( rma_pairset_t ) );
	place( &h.o_efn, sites.size() * sizeof( rma_efn_site_t ) );
	place( &h.o_pool, b.pool.size() );
	const size_t	match_at = at;		// (rms_match(): behind the pool, on the next multiple of 8)
	if( match ){
		h.flags |= RMS_IMG_MATCH;
		h.n_expr = int32_t( exprs.size() );
		if( !exprs.empty() )
			at += sizeof( RmsMatch ) + exprs.size() * sizeof( RmsMatchExpr ) + ops.size() * sizeof( RmqOp );
	}
	h.bytes = int32_t( at );
	if( text ){
		// the largest span two elements can enclose: every element at its longest, the contexts too
		int64_t	L = 0;
		for( int e = 0; e < prog.n_elems; e++ )
			L += std::max( 0, prog.elems[ e ].maxlen );
		if( prog.has_lctx ) L += std::max( 0, prog.lctx.maxlen );
		if( prog.has_rctx ) L += std::max( 0, prog.rctx.maxlen );
		h.flags |= RMS_IMG_TEXT;
		h.bits_L = int32_t( std::min<int64_t>( std::max<int64_t>( L, 1 ), RMS_BITS_MAX_L ) );
	}
	const int	wave = rms_wave_bytes( stack, h.n_vars );
	if( h.bytes + RMS_LDS_TABLES + wave > RMS_LDS_BYTES )
		return std::string( who ) + fmt( "an image of %d bytes and a wave's %d bytes of stack and variables leave no room for one wave in %d bytes of LDS",
			h.bytes, wave, int( RMS_LDS_BYTES ) );
	if( !exprs.empty() && h.bytes + RMS_LDS_TABLES + rms_wave_bytes( stack, h.n_vars, frames ) > RMS_LDS_BYTES )
		return std::string( who ) + fmt( "an image of %d bytes, a wave's %d bytes of stack and variables and the %d bytes of its matcher's %d frames leave no room "
			"for one wave in %d bytes of LDS", h.bytes, wave, rmq_wave_bytes( frames ), frames, int( RMS_LDS_BYTES ) );
	img.blob.assign( at / 8, 0 );
	char	*p = reinterpret_cast<char *>( img.blob.data() );
	auto put = [&]( int32_t o, const void *src, size_t bytes ){
		if( bytes > 0 )
			memcpy( p + o, src, bytes );
	};
	put( 0, &h, sizeof( h ) );
	put( h.o_dbl, b.dbl.data(), b.dbl.size() * sizeof( double ) );
	put( h.o_inst, b.inst.data(), b.inst.size() * sizeof( RmsInst ) );
	put( h.o_vars, b.vars.data(), b.vars.size() * sizeof( RmsVar ) );
	put( h.o_xd, xd.data(), xd.size() * sizeof( int32_t ) );
	put( h.o_rows, rows.data(), rows.size() * sizeof( RmsElem ) );
	put( h.o_ps, b.ps.data(), b.ps.size() * sizeof( rma_pairset_t ) );
	put( h.o_efn, sites.data(), sites.size() * sizeof( rma_efn_site_t ) );
	put( h.o_pool, b.pool.data(), b.pool.size() );
	if( !exprs.empty() ){
		const RmsMatch	mh{ int32_t( ops.size() ), frames };
		put( int32_t( match_at ), &mh, sizeof( mh ) );
		put( int32_t( match_at + sizeof( mh ) ), exprs.data(), exprs.size() * sizeof( RmsMatchExpr ) );
		put( int32_t( match_at + sizeof( mh ) + exprs.size() * sizeof( RmsMatchExpr ) ), ops.data(), ops.size() * sizeof( RmqOp ) );
	}
	img.prog.reset( new rma_program_t );
	memcpy( img.prog.get(), &prog, sizeof( rma_program_t ) );	// (every byte, padding too: rma_score_hits compares bytes)
	if( text ){
		// (the host VM's own expression, do_bits: its log10, its order of operations)
		img.bits_tab.reserve( size_t( h.bits_L ) * size_t( h.bits_L + 1 ) / 2 );
		for( int len = 1; len <= h.bits_L; len++ )
			for( int b = 1; b <= len; b++ )
				img.bits_tab.push_back( 3.32192809488736234789 * log10( 1.0 * b / len ) );
	}
	img.serial = ++serials;
	return "";
}

std::string score_stop_text( const ScoreImage &img, const RmsResult &r )
{
	const RmsImage	*m = img.image();
	const bool	in = r.pc >= 0 && r.pc < int( img.line_of.size() );
	const char	*f = in ? img.files[ size_t( img.file_of[ size_t( r.pc ) ] ) ].c_str() : " -- No File -- ";
	const int	l = in ? img.line_of[ size_t( r.pc ) ] : UNDEF;
	const char	*wd = img.wdfname.c_str();
	// (the rule's two string types are the VM's one)
	auto vm_type = []( int t ){ return t == RMS_T_BSTR || t == RMS_T_DEAD || t == RMS_T_HSTR ? int( T_STRING ) : t; };
	auto who = []( int sc ){ return sc == RMS_SC_BITS ? "bits" : sc == RMS_SC_EFN ? "efn" : sc == RMS_SC_MISMATCHES_1 ? "mismatches" : sc == RMS_SC_MISPAIRS ? "mispairs" : "paired"; };
	switch( r.stop ){
	case RMS_STOP_BUDGET : return fmt( "%s:%d more than %d instructions for one record (option score_budget).", f, l, r.a0 );
	case RMS_STOP_TYPE : return fmt( "%s:%d type mismatch.", f, l );
	case RMS_STOP_UNDEF_VAR :
		return fmt( "%s:%d variable '%s' is undefined.", f, l, r.a0 >= 0 && r.a0 < int( img.var_names.size() ) ? img.var_names[ size_t( r.a0 ) ].c_str() : "?" );
	case RMS_STOP_DIV_ZERO : return fmt( "%s:%d integer division by zero.", f, l );
	case RMS_STOP_DOLLAR : return fmt( "%s:%d '$' used outside a structure element reference.", f, l );
	case RMS_STOP_ESTK : return fmt( "%s:%d element stack overflow.", f, l );
	case RMS_STOP_STRCAT : return fmt( "%s:%d string + string needs a buffer, which a record on the device has not.", f, l );
	case RMS_STOP_SCORE_STRING : return fmt( "%s:%d SCORE holds a string: the device delivers an int or a float.", f, l );
	case RMS_STOP_STRF_NODESCR : return fmt( "%s:%d no such descr %d.", f, l, r.a0 );
	case RMS_STOP_STRF_POS_NEG : return fmt( "%s:%d bad pos %d, must be > 0.", f, l, r.a0 );
	case RMS_STOP_STRF_POS_BIG : return fmt( "%s:%d bad pos %d, must be <= %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_STRF_LEN : return fmt( "%s:%d bad len %d, must be > 0.", f, l, r.a0 );
	case RMS_STOP_INS_BASES : return fmt( "%s:%d pair has bad number of bases %d, requires %d-%d.", f, l, r.a0, 2, 4 );
	case RMS_STOP_INS_RHS : return fmt( "%s:%d rhs of \"in\" has wrong type %d, must be of type pairset (%d).", f, l, vm_type( r.a0 ), T_PAIRSET );
	case RMS_STOP_INS_ELEM : return fmt( "%s:%d pair elements must have type string.", f, l );
	case RMS_STOP_INS_LEN : return fmt( "%s:%d all pair elements must have the same length.", f, l );
	case RMS_STOP_INS_ARITY : return fmt( "%s:%d pair set arity does not match the number of elements.", f, l );
	case RMS_STOP_STRID_RANGE : return fmt( "%s:%d index %d out of range, must be between 1 and %d.", wd, UNDEF, r.a0, r.a1 );
	case RMS_STOP_STRID_TYPE : return fmt( "%s:%d descr type mismatch: have %s, need %s.", wd, UNDEF, strel_name( r.a0 ), strel_name( r.a1 ) );
	case RMS_STOP_STRID_TAG : {
		std::string	tag = "(bases of the record)";
		if( r.a0 == RMS_T_STRING && r.a1 >= 0 && r.a2 >= 0 && r.a1 + r.a2 <= m->n_pool )
			tag.assign( reinterpret_cast<const char *>( rms_pool( m ) ) + r.a1, size_t( r.a2 ) );
		return fmt( "%s:%d no such descr '%s'.", wd, UNDEF, tag.c_str() );
	}
	case RMS_STOP_XD : return fmt( "%s:%d %s: bad descr index %d, must be between 1 and %d.", f, l, who( r.a0 ), r.a1, r.a2 );
	case RMS_STOP_EFN_POS1_NEG : return fmt( "%s:%d efn: bad pos1 %d, must be > 0.", f, l, r.a0 );
	case RMS_STOP_EFN_LEN1 : return fmt( "%s:%d efn: descr1 must have a match len > 0.", f, l );
	case RMS_STOP_EFN_POS1_BIG : return fmt( "%s:%d efn: bad pos1 %d, must be <= %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_EFN_ORDER : return fmt( "%s:%d efn: bad 2nd descr index %d, must follow 1st descr %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_EFN_POS2_NEG : return fmt( "%s:%d efn: bad pos2 %d, must be > 0.", f, l, r.a0 );
	case RMS_STOP_EFN_LEN2 : return fmt( "%s:%d efn: descr2 must have a match len > 0.", f, l );
	case RMS_STOP_EFN_POS2_BIG : return fmt( "%s:%d efn: bad pos2 %d, must be <= %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_EFN_NO_VALUES : return fmt( "%s:%d efn(): no device energies for this candidate.", f, l );
	case RMS_STOP_EFN_NO_SITE : return fmt( "%s:%d efn(): call site was not registered with the scanner.", f, l );
	case RMS_STOP_LENGTH_ARG : return fmt( "%s:%d length: argument must be a string.", f, l );
	case RMS_STOP_LOC_RANGE : return fmt( "%s:%d descr index %d is out of range; must be between 1 and %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_LOC_POS_NEG : return fmt( "%s:%d loc: bad pos %d, must be > 0.", f, l, r.a0 );
	case RMS_STOP_LOC_LEN : return fmt( "%s:%d loc: bad matchlen %d, must be > 0.", f, l, r.a0 );
	case RMS_STOP_LOC_POS_BIG : return fmt( "%s:%d loc: bad pos %d, must be <= %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_PAIRED_POS : return fmt( "%s:%d paired: bad pos %d, must be between 1 and %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_PAIRED_LEN : return fmt( "%s:%d paired: bad len %d, must be > 0.", f, l, r.a0 );
	case RMS_STOP_PAIRED_SS : return "paired() does not accept descr type 'ss'.";
	case RMS_STOP_SUBSTR_POS : return fmt( "%s:%d substr: bad positiion %d, must be between 1 and %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_SUBSTR_LEN : return fmt( "%s:%d substr: bad len %d, must be >= 1.", f, l, r.a0 );
	case RMS_STOP_HEAP :
		return fmt( "%s:%d a string of %d bytes does not fit a record's heap: %d of its %d bytes are in use (option score_heap).", f, l, r.a0, r.a2, r.a1 );
	case RMS_STOP_TEXT_ROOM : return fmt( "%s:%d the score column has %d bytes, a row of the text has room for %d (text_stride).", f, l, r.a0, r.a1 );
	case RMS_STOP_TEXT_RANGE : return fmt( "%s:%d SCORE is not finite or not below 2^63: %%8.3lf of it is not written alike on host and device.", f, l );
	case RMS_STOP_SPF_FIRST : return fmt( "%s:%d sprintf: first argument must be a format string.", f, l );
	case RMS_STOP_SPF_BAD : {
		std::string	rest = "(a string made for the record)";
		if( r.a0 == RMS_T_STRING && r.a1 >= 0 && r.a2 >= 0 && r.a1 + r.a2 <= m->n_pool )
			rest.assign( reinterpret_cast<const char *>( rms_pool( m ) ) + r.a1, size_t( r.a2 ) );
		return fmt( "%s:%d sprintf: bad format '%s'.", f, l, rest.c_str() );
	}
	case RMS_STOP_SPF_STAR : return fmt( "%s:%d sprintf: '*' and '$' in formats are not supported by this build.", f, l );
	case RMS_STOP_SPF_NO_ARG : return fmt( "%s:%d No such argument %d.", f, l, r.a0 );
	case RMS_STOP_SPF_NEED_FLOAT : return fmt( "%s:%d '%c' format requires float arg.", f, l, r.a0 );
	case RMS_STOP_SPF_NEED_INT : return fmt( "%s:%d '%c' format requires int arg.", f, l, r.a0 );
	case RMS_STOP_SPF_NEED_STRING : return fmt( "%s:%d '%c' format requires string/seq arg.", f, l, r.a0 );
	case RMS_STOP_SPF_UNSUPPORTED : return fmt( "%s:%d '%c' unsupported format.", f, l, r.a0 );
	case RMS_STOP_SPF_EG : return fmt( "%s:%d sprintf: '%c' format: its digits are the host's C library's, the device writes %%f only.", f, l, r.a0 );
	case RMS_STOP_SPF_MODIFIER : return fmt( "%s:%d sprintf: '%c' format with something else than flags, a width and a precision.", f, l, r.a0 );
	case RMS_STOP_SPF_PREC : return fmt( "%s:%d sprintf: a precision of %d, the device writes at most %d digits behind the point.", f, l, r.a0, int( RMS_FMT_MAX_PREC ) );
	case RMS_STOP_SPF_RANGE : return fmt( "%s:%d sprintf: 'f' format of a float that is not finite or not below 2^63.", f, l );
	case RMS_STOP_BITS_POS1_NEG : return fmt( "%s:%d bits: bad pos1 %d, must be > 0.", f, l, r.a0 );
	case RMS_STOP_BITS_LEN1 : return fmt( "%s:%d bits: descr1 must have match len > 0.", f, l );
	case RMS_STOP_BITS_POS1_BIG : return fmt( "%s:%d bits: bad pos1 %d, must be <= %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_BITS_ORDER : return fmt( "%s:%d bits: bad 2nd descr index %d, must follow 1st descr index %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_BITS_POS2_NEG : return fmt( "%s:%d bits: bad pas2 %d, must be > 0", f, l, r.a0 );
	case RMS_STOP_BITS_LEN2 : return fmt( "%s:%d bits: descr2 must have match len > 0.", f, l );
	case RMS_STOP_BITS_POS2_BIG : return fmt( "%s:%d bits: bad pos2 %d, must be <= %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_BITS_SPAN : return fmt( "%s:%d bits() over %d bases, the table of its logarithms ends at %d.", f, l, r.a0, r.a1 );
	case RMS_STOP_MAT_TYPE : return fmt( "%s:%d typemismatch.", f, l );
	default :
		return fmt( "%s:%d the image holds what the rule does not run (stop %d, %d).", f, l, r.stop, r.a0 );
	}
}

}	// namespace rma
