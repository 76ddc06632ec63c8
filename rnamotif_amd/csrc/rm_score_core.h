// rm_score_core.h -- the score section's MAIN program on one hit record: one rule for the host (tests/hostsim/score_check.cpp,
// the words of a stop in rm_score_image.cpp) and the device (rma_score_kernel, rm_score_dev.hip).
//
// rms_run() restates ScoreVM::run, do_compare, do_arith, do_incr, do_strf, do_scl, strid, paired and do_efn of rm_score.cpp
// instruction for instruction over an image (rm_score_image.h), oddities included: an int operand keeps its type under
// int op float; && and || on a float leave the slot typed float with its low word overwritten; $ reads rm_descr, not
// rm_xdescr; a failing quad is paired; do_efn tests pos where pos2 is meant; the value of efn() is float( 0.01 * word ).
//
// No string is copied.  A string value is a slice -- offset and length -- of the record's strand (RMS_T_BSTR), read through
// the accessor `bases`, or of the image's pool (RMS_T_STRING).  Element references and substr() cut slices, string
// variables hold them, length(), the comparisons (strcmp's order) and `in` read them in place.  String + needs a buffer
// and stops.  Every fail() of the host VM that a record can reach stops with a code of its own and up to three numbers;
// rms_stop_text() (rm_score_image.cpp) makes the host VM's words of them.  One stop the host VM does not have: more
// than `budget` instructions for one record.
//
// An image opened with RMS_IMG_TEXT (rm_score_image.h) has a third string type, RMS_T_HSTR: a slice of the lane's heap,
// an arena of `heap_cap` bytes a record that only grows (RmsMem::HB; on the device dwords interleaved by lane in global
// memory).  String + concatenates into it, sprintf() (do_sprintf, directive for directive, through rm_score_fmt.h)
// writes into it, bits() (do_bits) reads its logarithms from the image's table (RmsText::bits_tab), and a string in
// SCORE at ACCEPT is kind 3.  With a row to write (RmsText::row) ACCEPT leaves the score column HitPrinter::print
// writes: %8d, %8.3lf or %8s.  Every directive on which the host VM only notes an error stops here.  rms_run_t< false >
// is the rule without any of this, what rms_run() is.
//
// An image opened with RMS_IMG_MATCH holds =~ / !~ (MAT; !~ is MAT and NOT) and mismatches( string, pattern ), each with
// the index of an expression the image has compiled (RmsMatch): rms_run_t< TEXT, true > runs do_mat and the builtin through
// rmq_step() and rmq_mm_step() of rm_seqcheck.h -- the reference's step(), advance() and mm_step() -- over the left
// operand, a string of any of the three types read through an accessor that ends it with a 0 at its length and reads
// nothing behind it.  The pattern on the stack is the constant the expression was compiled from and is not read.  The
// matcher's frames and its bra[] / ket[] are planes of their own (RmsMem::mq: an RmqMem); every op it visits counts
// against the record's budget with the instructions.  MAT on something that is no string stops with the host VM's word
// for it, "typemismatch.".
//
// Where the host VM would read what it has freed or never wrote -- a string slot after && / || / ! (its pointer's low
// word is overwritten), substr() of something that is no string, $ on an entry of rm_xdescr behind rm_descr's end --
// the rule stops with "type mismatch" or the $ stop.  The value an assignment leaves on the stack is the host's
// identifier slot, whose int view is the low word of a pointer: here 1, like it never 0 -- a chained assignment, y = x = 5,
// which stores that word, is the one place where the two sides differ (the host's value is no number of the program's).
//
// The lane's state lives in planes (RmsMem): slot k's three words at ( 3 k + j ) * STRIDE -- STRIDE 1 on the host, 64 in
// LDS, where the 64 lanes of a wave then touch 64 consecutive words.  Indices are clamped into the planes: a program
// the analysis of hit_independent() passed never needs that, and no other can reach memory that is not the lane's.
#pragma once
#include <cstdint>
#include <cstring>
#include "rm_score_image.h"
#include "rm_score_fmt.h"

#ifndef RMD_FN
#define RMD_FN	static inline
#endif
#ifndef RMD_FN_MEMBER
#define RMD_FN_MEMBER	inline
#endif

// value types: T_* of rm_host.h, then the rule's own
enum { RMS_T_UNDEF, RMS_T_INT, RMS_T_FLOAT, RMS_T_STRING, RMS_T_PAIRSET, RMS_T_POS, RMS_T_IDENT, RMS_T_HIT,
	RMS_T_BSTR,		// a string: a slice of the record's strand
	RMS_T_DEAD,		// a string slot whose pointer && / || / ! overwrote: only its int view is left
	RMS_T_HSTR		// a string: a slice of the lane's heap
};
// op codes and builtins: OP_* and SC_* of rm_score.h
enum {
	RMS_OP_HALT, RMS_OP_NOOP, RMS_OP_ACPT, RMS_OP_HOLD, RMS_OP_RJCT, RMS_OP_RLSE, RMS_OP_MRK, RMS_OP_CLS, RMS_OP_FCL, RMS_OP_SCL,
	RMS_OP_STRF, RMS_OP_LDA, RMS_OP_LOD, RMS_OP_LDC, RMS_OP_STO, RMS_OP_AND, RMS_OP_IOR, RMS_OP_NOT, RMS_OP_MAT, RMS_OP_INS,
	RMS_OP_GTR, RMS_OP_GEQ, RMS_OP_EQU, RMS_OP_NEQ, RMS_OP_LEQ, RMS_OP_LES, RMS_OP_ADD, RMS_OP_SUB, RMS_OP_MUL, RMS_OP_DIV,
	RMS_OP_MOD, RMS_OP_NEG, RMS_OP_I_PP, RMS_OP_PP_I, RMS_OP_I_MM, RMS_OP_MM_I, RMS_OP_FJP, RMS_OP_JMP, RMS_N_OP
};
enum {
	RMS_SC_STRID, RMS_SC_BITS, RMS_SC_EFN, RMS_SC_EFN2, RMS_SC_LENGTH, RMS_SC_LOC, RMS_SC_MISMATCHES, RMS_SC_MISMATCHES_1,
	RMS_SC_MISMATCHES_2, RMS_SC_MISPAIRS, RMS_SC_PAIRED, RMS_SC_SPRINTF, RMS_SC_SUBSTR, RMS_N_SC
};

enum { RMS_REJECT, RMS_ACCEPT, RMS_STOPPED };
enum { RMS_KIND_NONE, RMS_KIND_INT, RMS_KIND_FLOAT, RMS_KIND_STRING };

// why a record stopped; a0, a1, a2 as the words need them (rms_stop_text)
enum {
	RMS_STOP_NONE,
	RMS_STOP_BUDGET,		// a0: the budget
	RMS_STOP_TYPE,			// "type mismatch."
	RMS_STOP_UNDEF_VAR,		// a0: the variable
	RMS_STOP_DIV_ZERO,
	RMS_STOP_DOLLAR,		// $ outside a reference (or on an entry behind rm_descr's end)
	RMS_STOP_ESTK,			// element stack overflow
	RMS_STOP_STRCAT,		// string + string
	RMS_STOP_SCORE_STRING,		// ACCEPT with a string in SCORE: the call delivers numbers
	RMS_STOP_INTERNAL,		// an instruction the image should not hold, a pc or stack outside the program's
	RMS_STOP_STRF_NODESCR,		// a0: index
	RMS_STOP_STRF_POS_NEG,		// a0: pos
	RMS_STOP_STRF_POS_BIG,		// a0: pos, a1: matchlen
	RMS_STOP_STRF_LEN,		// a0: len
	RMS_STOP_INS_BASES,		// a0: operands
	RMS_STOP_INS_RHS,		// a0: type
	RMS_STOP_INS_ELEM,
	RMS_STOP_INS_LEN,
	RMS_STOP_INS_ARITY,
	RMS_STOP_STRID_RANGE,		// a0: index, a1: entries
	RMS_STOP_STRID_TYPE,		// a0: have, a1: need (as the host VM names them)
	RMS_STOP_STRID_TAG,		// a0: string type, a1: offset, a2: length
	RMS_STOP_XD,			// a0: builtin, a1: index + 1, a2: entries
	RMS_STOP_EFN_POS1_NEG, RMS_STOP_EFN_LEN1, RMS_STOP_EFN_POS1_BIG, RMS_STOP_EFN_ORDER, RMS_STOP_EFN_POS2_NEG, RMS_STOP_EFN_LEN2,
	RMS_STOP_EFN_POS2_BIG, RMS_STOP_EFN_NO_VALUES, RMS_STOP_EFN_NO_SITE,
	RMS_STOP_LENGTH_ARG,
	RMS_STOP_LOC_RANGE, RMS_STOP_LOC_POS_NEG, RMS_STOP_LOC_LEN, RMS_STOP_LOC_POS_BIG,
	RMS_STOP_PAIRED_POS, RMS_STOP_PAIRED_LEN, RMS_STOP_PAIRED_SS,
	RMS_STOP_SUBSTR_POS, RMS_STOP_SUBSTR_LEN,
	// an image with RMS_IMG_TEXT
	RMS_STOP_HEAP,			// a0: bytes asked for, a1: score_heap, a2: bytes in use
	RMS_STOP_TEXT_ROOM,		// a0: the score column's length, a1: text_stride
	RMS_STOP_TEXT_RANGE,		// SCORE is a float %8.3lf cannot be written alike on host and device
	RMS_STOP_SPF_FIRST,		// sprintf: the first argument is no string
	RMS_STOP_SPF_BAD,		// no conversion letter; a0: string type, a1: offset, a2: length of the format's rest
	RMS_STOP_SPF_STAR,		// * or $
	RMS_STOP_SPF_NO_ARG,		// a0: the argument
	RMS_STOP_SPF_NEED_FLOAT, RMS_STOP_SPF_NEED_INT, RMS_STOP_SPF_NEED_STRING, RMS_STOP_SPF_UNSUPPORTED,	// a0: the letter
	RMS_STOP_SPF_EG,		// a0: the letter, one of e E g G
	RMS_STOP_SPF_MODIFIER,		// a0: the letter
	RMS_STOP_SPF_PREC,		// a0: the precision
	RMS_STOP_SPF_RANGE,		// %f of a double that is not finite or not below 2^63
	RMS_STOP_BITS_POS1_NEG, RMS_STOP_BITS_LEN1, RMS_STOP_BITS_POS1_BIG, RMS_STOP_BITS_ORDER, RMS_STOP_BITS_POS2_NEG, RMS_STOP_BITS_LEN2,
	RMS_STOP_BITS_POS2_BIG,
	RMS_STOP_BITS_SPAN,		// a0: bases, a1: the table's L
	// an image with RMS_IMG_MATCH
	RMS_STOP_MAT_TYPE,		// =~ / !~ on something that is no string: "typemismatch."
	RMS_N_STOP
};

struct RmsResult {
	int32_t	outcome;	// RMS_REJECT, RMS_ACCEPT, RMS_STOPPED
	int32_t	kind;		// of SCORE, for an accepted record
	double	score;		// an int SCORE as its exact double
	int32_t	stop, pc, a0, a1, a2;
	int32_t	text_len;	// bytes of the score column in RmsText::row
};

// what the rule of an image with RMS_IMG_TEXT reads and writes beside the planes
struct RmsText {
	const double	*bits_tab = nullptr;	// 3.32... * log10( b / len ) at ( len - 1 ) * len / 2 + b - 1, 1 <= b <= len <= RmsImage::bits_L
	uint8_t	*row = nullptr;		// not null: where ACCEPT writes the score column, row_cap bytes
	int	row_cap = 0;
};

// the parts of an image
RMD_FN const RmsInst *rms_inst( const RmsImage *m ) { return reinterpret_cast<const RmsInst *>( reinterpret_cast<const char *>( m ) + m->o_inst ); }
RMD_FN const double *rms_dbl( const RmsImage *m ) { return reinterpret_cast<const double *>( reinterpret_cast<const char *>( m ) + m->o_dbl ); }
RMD_FN const RmsVar *rms_vars( const RmsImage *m ) { return reinterpret_cast<const RmsVar *>( reinterpret_cast<const char *>( m ) + m->o_vars ); }
RMD_FN const int32_t *rms_xd( const RmsImage *m ) { return reinterpret_cast<const int32_t *>( reinterpret_cast<const char *>( m ) + m->o_xd ); }
RMD_FN const RmsElem *rms_rows( const RmsImage *m ) { return reinterpret_cast<const RmsElem *>( reinterpret_cast<const char *>( m ) + m->o_rows ); }
RMD_FN const rma_pairset_t *rms_ps( const RmsImage *m ) { return reinterpret_cast<const rma_pairset_t *>( reinterpret_cast<const char *>( m ) + m->o_ps ); }
RMD_FN const rma_efn_site_t *rms_efn( const RmsImage *m ) { return reinterpret_cast<const rma_efn_site_t *>( reinterpret_cast<const char *>( m ) + m->o_efn ); }
RMD_FN const unsigned char *rms_pool( const RmsImage *m ) { return reinterpret_cast<const unsigned char *>( m ) + m->o_pool; }

// A lane's planes: `stack` slots, behind them n_vars variables, three words each; the element stack a byte a slot.
template< int STRIDE > struct RmsMem {
	int32_t	*w;
	uint8_t	*e;
	int	stack, n_vars;
	uint8_t	*heap = nullptr;	// the lane's arena: byte k at ( k >> 2 ) * 4 * STRIDE + ( k & 3 )
	int	heap_cap = 0;
	int32_t	*mq = nullptr;		// the matcher's planes (RmqMem< STRIDE >, rm_seqcheck.h), mq_frames frames of them
	int	mq_frames = 0;
	static constexpr int	stride = STRIDE;
	RMD_FN_MEMBER uint8_t	&HB( int k ) const { return heap[ ( ( k < 0 ? 0 : k >= heap_cap ? heap_cap - 1 : k ) >> 2 ) * 4 * STRIDE + ( k & 3 ) ]; }
	RMD_FN_MEMBER int	slot( int k ) const { return k < 0 ? 0 : k >= stack ? stack - 1 : k; }
	RMD_FN_MEMBER int	var( int v ) const { return stack + ( v < 0 ? 0 : v >= n_vars ? n_vars - 1 : v ); }
	RMD_FN_MEMBER int32_t	&T( int k ) const { return w[ ( 3 * slot( k ) ) * STRIDE ]; }
	RMD_FN_MEMBER int32_t	&L( int k ) const { return w[ ( 3 * slot( k ) + 1 ) * STRIDE ]; }
	RMD_FN_MEMBER int32_t	&H( int k ) const { return w[ ( 3 * slot( k ) + 2 ) * STRIDE ]; }
	RMD_FN_MEMBER int32_t	&VT( int v ) const { return w[ ( 3 * var( v ) ) * STRIDE ]; }
	RMD_FN_MEMBER int32_t	&VL( int v ) const { return w[ ( 3 * var( v ) + 1 ) * STRIDE ]; }
	RMD_FN_MEMBER int32_t	&VH( int v ) const { return w[ ( 3 * var( v ) + 2 ) * STRIDE ]; }
	RMD_FN_MEMBER uint8_t	&E( int k ) const { return e[ ( k < 0 ? 0 : k >= RMS_ESTK ? RMS_ESTK - 1 : k ) * STRIDE ]; }
};

RMD_FN double rms_double( int32_t lo, int32_t hi )
{
	const uint64_t	u = ( uint64_t( uint32_t( hi ) ) << 32 ) | uint32_t( lo );
	double	d;
	memcpy( &d, &u, sizeof( d ) );
	return d;
}
RMD_FN void rms_words( double d, int32_t *lo, int32_t *hi )
{
	uint64_t	u;
	memcpy( &u, &d, sizeof( u ) );
	*lo = int32_t( uint32_t( u ) );
	*hi = int32_t( uint32_t( u >> 32 ) );
}

RMD_FN int rms_is_string( int t ) { return t == RMS_T_STRING || t == RMS_T_BSTR || t == RMS_T_HSTR; }

// b2bc[], compile.c:180-187
RMD_FN int rms_b2bc( unsigned char c )
{
	switch( c ){
	case 'a' : case 'A' : return RMA_BC_A;
	case 'c' : case 'C' : return RMA_BC_C;
	case 'g' : case 'G' : return RMA_BC_G;
	case 't' : case 'T' : case 'u' : case 'U' : return RMA_BC_T;
	default : return RMA_BC_N;
	}
}

// byte i of a string value
template< class Bases > RMD_FN unsigned char rms_char( const RmsImage *m, const Bases &bases, int type, int off, int i )
{
	if( type == RMS_T_BSTR )
		return bases( off + i );
	const unsigned	at = unsigned( off ) + unsigned( i );
	return at < unsigned( m->n_pool ) ? rms_pool( m )[ at ] : 0;
}

// strcmp's sign over two slices
template< class Bases > RMD_FN int rms_strcmp( const RmsImage *m, const Bases &bases, int t1, int o1, int n1, int t2, int o2, int n2 )
{
	const int	n = n1 < n2 ? n1 : n2;
	for( int i = 0; i < n; i++ ){
		const int	a = rms_char( m, bases, t1, o1, i ), b = rms_char( m, bases, t2, o2, i );
		if( a != b )
			return a < b ? -1 : 1;
	}
	return n1 < n2 ? -1 : n1 > n2;
}

// the same with the heap's slices; TEXT false: the two above
template< bool TEXT, class Mem, class Bases > RMD_FN unsigned char rms_char_t( const RmsImage *m, const Bases &bases, const Mem &mem, int type, int off, int i )
{
	if( TEXT && type == RMS_T_HSTR ){
		const unsigned	at = unsigned( off ) + unsigned( i );
		return at < unsigned( mem.heap_cap ) ? mem.HB( int( at ) ) : 0;
	}
	return rms_char( m, bases, type, off, i );
}
template< bool TEXT, class Mem, class Bases >
RMD_FN int rms_strcmp_t( const RmsImage *m, const Bases &bases, const Mem &mem, int t1, int o1, int n1, int t2, int o2, int n2 )
{
	if( !TEXT )
		return rms_strcmp( m, bases, t1, o1, n1, t2, o2, n2 );
	const int	n = n1 < n2 ? n1 : n2;
	for( int i = 0; i < n; i++ ){
		const int	a = rms_char_t<TEXT>( m, bases, mem, t1, o1, i ), b = rms_char_t<TEXT>( m, bases, mem, t2, o2, i );
		if( a != b )
			return a < b ? -1 : 1;
	}
	return n1 < n2 ? -1 : n1 > n2;
}

// the bytes of a string value, for the formatter
template< bool TEXT, class Mem, class Bases > struct RmsStr {
	const RmsImage	*m;
	const Bases	&bases;
	const Mem	&mem;
	int	type, off;
	RMD_FN_MEMBER unsigned char	operator()( int i ) const { return rms_char_t<TEXT>( m, bases, mem, type, off, i ); }
};

// a string value as the matcher's text: byte k of the slice, 0 at its length and wherever else it is asked
template< bool TEXT, class Mem, class Bases > struct RmsMatchText {
	const RmsImage	*m;
	const Bases	&bases;
	const Mem	&mem;
	int	type, off, len;
	RMD_FN_MEMBER int	operator()( int k ) const { return unsigned( k ) < unsigned( len ) ? int( rms_char_t<TEXT>( m, bases, mem, type, off, k ) ) : 0; }
};

// where a row of the element table has its offset and length in the record
RMD_FN int rms_row_word( const RmsImage *m, int row )
{
	return row < m->n_elems ? RMA_HIT_HDR + 4 * row : m->ctx_off + 2 * ( row - m->n_elems );
}

// The rule.  w: the record; slen: its entry's length; bases( i ): the letter at position i of the record's strand;
// mem: the lane's planes, sized for m->stack slots and m->n_vars variables.
template< bool TEXT, bool MATCH = false, class Mem, class Bases >
RMD_FN void rms_run_t( const RmsImage *m, const int32_t *w, int slen, const Bases &bases, const Mem &mem, int budget, RmsResult *r, const RmsText &tx )
{
	const bool	text = TEXT && ( m->flags & RMS_IMG_TEXT ) != 0;
	int	hp = 0;		// bytes of the heap in use
	const RmsInst	*prog = rms_inst( m );
	const int32_t	*xd = rms_xd( m );
	const RmsElem	*rows = rms_rows( m );
	const int	n_xd = m->n_xd;
	int	pc = 0, sp = -1, mp = -1, esp = -1, steps = 0;
	r->outcome = RMS_REJECT;
	r->kind = RMS_KIND_NONE;
	r->score = 0.0;
	r->stop = RMS_STOP_NONE;
	r->pc = r->a0 = r->a1 = r->a2 = 0;
	r->text_len = 0;
#define RMS_STOP( code, x, y, z )	do{ r->outcome = RMS_STOPPED; r->stop = ( code ); r->pc = pc - 1; r->a0 = ( x ); r->a1 = ( y ); r->a2 = ( z ); return; }while( 0 )
#define RMS_MLEN( row )	( w[ rms_row_word( m, ( row ) ) + 1 ] )
#define RMS_MOFF( row )	( w[ rms_row_word( m, ( row ) ) ] )
	// the variables as BEGIN left them; NAME COMP POS LEN as find_ss sets them (Replayer::one_hit), SLEN as run() does
	{
		const RmsVar	*v0 = rms_vars( m );
		for( int v = 0; v < m->n_vars; v++ ){
			mem.VT( v ) = v0[ v ].type;
			mem.VL( v ) = v0[ v ].lo;
			mem.VH( v ) = v0[ v ].hi;
		}
		const int	comp = w[ 1 ];
		if( m->v_comp >= 0 )
			mem.VL( m->v_comp ) = comp;
		if( m->v_pos >= 0 )
			mem.VL( m->v_pos ) = comp ? slen - w[ RMA_HIT_HDR ] : w[ RMA_HIT_HDR ] + 1;
		if( m->v_len >= 0 ){
			int	len = 0;
			for( int e = 0; e < m->n_elems; e++ )
				len += w[ RMA_HIT_HDR + 4 * e + 1 ];
			mem.VL( m->v_len ) = len;
		}
		if( m->v_slen >= 0 )
			mem.VL( m->v_slen ) = slen;
	}
	if( m->n_inst == 0 )
		goto accept;
	for( ; ; ){
		if( pc < 0 || pc >= m->n_inst ){
			pc++;
			RMS_STOP( RMS_STOP_INTERNAL, 0, 0, 0 );
		}
		const RmsInst	ip = prog[ pc++ ];
		if( ++steps > budget )
			RMS_STOP( RMS_STOP_BUDGET, budget, 0, 0 );
		if( sp + 2 > mem.stack )
			RMS_STOP( RMS_STOP_INTERNAL, 1, 0, 0 );
		switch( ip.op ){
		case RMS_OP_NOOP :
			break;
		case RMS_OP_ACPT :
			goto accept;
		case RMS_OP_RJCT :
			return;
		case RMS_OP_MRK :
			sp++;
			mem.T( sp ) = RMS_T_INT;
			mem.L( sp ) = mp;
			mp = sp;
			break;
		case RMS_OP_CLS :
			sp = mp = -1;
			break;
		case RMS_OP_LDA :
			sp++;
			mem.T( sp ) = RMS_T_IDENT;
			mem.L( sp ) = ip.a;
			break;
		case RMS_OP_LOD : {		// do_lod
			const int	t = mem.VT( ip.a );
			if( t == RMS_T_UNDEF )
				RMS_STOP( RMS_STOP_UNDEF_VAR, ip.a, 0, 0 );
			if( t != RMS_T_INT && t != RMS_T_FLOAT && !rms_is_string( t ) )
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			sp++;
			mem.T( sp ) = t;
			mem.L( sp ) = mem.VL( ip.a );
			mem.H( sp ) = mem.VH( ip.a );
			break;
		}
		case RMS_OP_LDC :		// do_ldc
			sp++;
			switch( ip.kind ){
			case RMS_K_INT :
				mem.T( sp ) = RMS_T_INT;
				mem.L( sp ) = ip.a;
				break;
			case RMS_K_FLOAT : {
				int32_t	lo, hi;
				rms_words( rms_dbl( m )[ ip.a ], &lo, &hi );
				mem.T( sp ) = RMS_T_FLOAT;
				mem.L( sp ) = lo;
				mem.H( sp ) = hi;
				break;
			}
			case RMS_K_STRING :
				mem.T( sp ) = RMS_T_STRING;
				mem.L( sp ) = ip.a;
				mem.H( sp ) = ip.len;
				break;
			case RMS_K_POS : {
				if( esp < 0 )
					RMS_STOP( RMS_STOP_DOLLAR, 0, 0, 0 );
				const int	e = mem.E( esp );		// (sic) an index of rm_xdescr, applied to rm_descr
				if( e >= m->n_elems )
					RMS_STOP( RMS_STOP_DOLLAR, 0, 0, 0 );
				mem.T( sp ) = RMS_T_INT;
				mem.L( sp ) = w[ RMA_HIT_HDR + 4 * e + 1 ];
				break;
			}
			case RMS_K_PAIRSET :
				mem.T( sp ) = RMS_T_PAIRSET;
				mem.L( sp ) = ip.a;
				break;
			default :
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			}
			break;
		case RMS_OP_STO : {		// do_sto
			const int	top = sp--;
			if( mem.T( sp ) != RMS_T_IDENT )
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			const int	v = mem.L( sp ), vt = mem.VT( v ), tt = mem.T( top );
			if( vt == RMS_T_UNDEF && ( tt == RMS_T_INT || tt == RMS_T_FLOAT ) ){
				mem.T( sp ) = tt;
				mem.VT( v ) = tt;
				mem.VL( v ) = mem.L( top );
				mem.VH( v ) = mem.H( top );
			}else if( ( vt == RMS_T_UNDEF || rms_is_string( vt ) ) && rms_is_string( tt ) ){
				mem.VT( v ) = tt;
				mem.VL( v ) = mem.L( top );
				mem.VH( v ) = mem.H( top );
			}else if( vt == RMS_T_INT && tt == RMS_T_INT )
				mem.VL( v ) = mem.L( top );
			else if( vt == RMS_T_INT && tt == RMS_T_FLOAT )
				mem.VL( v ) = int( rms_double( mem.L( top ), mem.H( top ) ) );
			else if( vt == RMS_T_FLOAT && ( tt == RMS_T_INT || tt == RMS_T_FLOAT ) ){
				const double	d = tt == RMS_T_INT ? double( mem.L( top ) ) : rms_double( mem.L( top ), mem.H( top ) );
				int32_t	lo, hi;
				rms_words( d, &lo, &hi );
				mem.VL( v ) = lo;
				mem.VH( v ) = hi;
			}else
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			mem.L( sp ) = 1;		// (the low word of the identifier's address)
			break;
		}
		case RMS_OP_AND :
		case RMS_OP_IOR : {		// do_and, do_ior
			const int	t = mem.T( sp );
			int	rv;
			if( t == RMS_T_INT )
				rv = mem.L( sp ) != 0;
			else if( t == RMS_T_FLOAT )
				rv = rms_double( mem.L( sp ), mem.H( sp ) ) != 0.0;	// (sic) the type stays float
			else if( rms_is_string( t ) ){
				rv = mem.H( sp ) > 0;
				mem.T( sp ) = RMS_T_DEAD;
			}else
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			mem.L( sp ) = rv;
			if( ip.op == RMS_OP_AND ? !rv : rv )
				pc = ip.a;
			break;
		}
		case RMS_OP_NOT : {		// do_not
			const int	t = mem.T( sp );
			if( t == RMS_T_INT )
				mem.L( sp ) = !( mem.L( sp ) != 0 );
			else if( t == RMS_T_FLOAT )
				mem.L( sp ) = !( rms_double( mem.L( sp ), mem.H( sp ) ) != 0.0 );
			else if( rms_is_string( t ) ){
				mem.L( sp ) = !( mem.H( sp ) > 0 );
				mem.T( sp ) = RMS_T_DEAD;
			}else
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			break;
		}
		case RMS_OP_MAT : {		// do_mat
			if( !MATCH || !( m->flags & RMS_IMG_MATCH ) || unsigned( ip.a ) >= unsigned( m->n_expr ) )
				RMS_STOP( RMS_STOP_INTERNAL, 8, 0, 0 );
			const int	top = sp--;
			if( sp < 0 )
				RMS_STOP( RMS_STOP_INTERNAL, 9, 0, 0 );
			const int	t1 = mem.T( sp ), t2 = mem.T( top );
			if( !( rms_is_string( t1 ) || t1 == RMS_T_DEAD ) || !( rms_is_string( t2 ) || t2 == RMS_T_DEAD ) )
				RMS_STOP( RMS_STOP_MAT_TYPE, 0, 0, 0 );
			if( t1 == RMS_T_DEAD )		// (the host reads a pointer && / || / ! overwrote)
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			const RmsMatchExpr	ex = rms_match_expr( m )[ ip.a ];
			int	rv = 0;
			if( ex.n_ops >= 0 ){
				const RmsMatchText<TEXT, Mem, Bases>	text{ m, bases, mem, t1, mem.L( sp ), mem.H( sp ) };
				const RmqMem<Mem::stride>	mq{ mem.mq, mem.mq_frames };
				rv = rmq_step( rms_match_ops( m ) + ex.first, ex.n_ops, text, mq, ex.anchored != 0, budget, &steps );
				if( rv < 0 )
					RMS_STOP( RMS_STOP_BUDGET, budget, 0, 0 );
			}
			mem.T( sp ) = RMS_T_INT;
			mem.L( sp ) = rv;
			break;
		}
		case RMS_OP_INS : {		// do_ins
			const int	n_bases = sp - mp - 1;
			if( n_bases < 2 || n_bases > 4 )
				RMS_STOP( RMS_STOP_INS_BASES, n_bases, 0, 0 );
			if( mem.T( sp ) != RMS_T_PAIRSET )
				RMS_STOP( RMS_STOP_INS_RHS, mem.T( sp ), 0, 0 );
			const unsigned	pi = unsigned( mem.L( sp ) );
			if( pi >= unsigned( m->n_ps ) )
				RMS_STOP( RMS_STOP_INTERNAL, 2, 0, 0 );
			const rma_pairset_t	*ps = rms_ps( m ) + pi;
			int	l0 = -1;
			for( int i = 0; i < n_bases; i++ ){
				if( !rms_is_string( mem.T( mp + 1 + i ) ) )
					RMS_STOP( RMS_STOP_INS_ELEM, 0, 0, 0 );
				const int	l = mem.H( mp + 1 + i );
				if( l0 == -1 )
					l0 = l;
				else if( l != l0 )
					RMS_STOP( RMS_STOP_INS_LEN, 0, 0, 0 );
			}
			int	rv = 1;
			for( int i = 0; i < l0 && rv; i++ ){
				int	ix = 0;
				for( int k = 0; k < n_bases; k++ )
					ix = ix * 5 + rms_b2bc( rms_char_t<TEXT>( m, bases, mem, mem.T( mp + 1 + k ), mem.L( mp + 1 + k ), i ) );
				if( n_bases == 2 )
					rv = ( ps->mat2 >> ix ) & 1;
				else if( n_bases == 3 )
					rv = ( ps->mat3[ ix >> 5 ] >> ( ix & 31 ) ) & 1;
				else
					rv = ( ps->mat4[ ix >> 5 ] >> ( ix & 31 ) ) & 1;
				if( ps->n_bases != n_bases )
					RMS_STOP( RMS_STOP_INS_ARITY, 0, 0, 0 );
			}
			sp = mp;
			mp = mem.L( mp );
			mem.T( sp ) = RMS_T_INT;
			mem.L( sp ) = rv;
			break;
		}
		case RMS_OP_GTR : case RMS_OP_GEQ : case RMS_OP_EQU : case RMS_OP_NEQ : case RMS_OP_LEQ : case RMS_OP_LES : {	// do_compare
			const int	top = sp--;
			const int	t1 = mem.T( sp ), t2 = mem.T( top );
			int	c;	// sign of the comparison, or 2 for unordered
			if( t1 == RMS_T_INT && t2 == RMS_T_INT ){
				const int	a = mem.L( sp ), b = mem.L( top );
				c = a < b ? -1 : a > b;
			}else if( ( t1 == RMS_T_INT || t1 == RMS_T_FLOAT ) && ( t2 == RMS_T_INT || t2 == RMS_T_FLOAT ) ){
				const double	a = t1 == RMS_T_INT ? double( mem.L( sp ) ) : rms_double( mem.L( sp ), mem.H( sp ) );
				const double	b = t2 == RMS_T_INT ? double( mem.L( top ) ) : rms_double( mem.L( top ), mem.H( top ) );
				c = a < b ? -1 : a > b ? 1 : a == b ? 0 : 2;
			}else if( rms_is_string( t1 ) && rms_is_string( t2 ) )
				c = rms_strcmp_t<TEXT>( m, bases, mem, t1, mem.L( sp ), mem.H( sp ), t2, mem.L( top ), mem.H( top ) );
			else
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			int	rv;
			switch( ip.op ){
			case RMS_OP_GTR : rv = c == 1; break;
			case RMS_OP_GEQ : rv = c == 1 || c == 0; break;
			case RMS_OP_EQU : rv = c == 0; break;
			case RMS_OP_NEQ : rv = c != 0; break;
			case RMS_OP_LEQ : rv = c == -1 || c == 0; break;
			default : rv = c == -1; break;
			}
			mem.T( sp ) = RMS_T_INT;
			mem.L( sp ) = rv;
			break;
		}
		case RMS_OP_ADD : case RMS_OP_SUB : case RMS_OP_MUL : case RMS_OP_DIV : case RMS_OP_MOD : {	// do_arith
			const int	top = sp--;
			const int	t1 = mem.T( sp ), t2 = mem.T( top ), op = ip.op;
			if( t1 == RMS_T_INT && t2 == RMS_T_INT ){
				const int32_t	a = mem.L( sp ), b = mem.L( top );
				int32_t	v;
				if( ( op == RMS_OP_DIV || op == RMS_OP_MOD ) && b == 0 )
					RMS_STOP( RMS_STOP_DIV_ZERO, 0, 0, 0 );
				switch( op ){
				case RMS_OP_ADD : v = int32_t( uint32_t( a ) + uint32_t( b ) ); break;
				case RMS_OP_SUB : v = int32_t( uint32_t( a ) - uint32_t( b ) ); break;
				case RMS_OP_MUL : v = int32_t( uint32_t( a ) * uint32_t( b ) ); break;
				case RMS_OP_DIV : v = b == -1 ? int32_t( 0u - uint32_t( a ) ) : a / b; break;
				default : v = b == -1 ? 0 : a % b; break;
				}
				mem.L( sp ) = v;
			}else if( ( t1 == RMS_T_INT || t1 == RMS_T_FLOAT ) && ( t2 == RMS_T_INT || t2 == RMS_T_FLOAT ) ){
				if( op == RMS_OP_MOD )
					RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
				const double	a = t1 == RMS_T_INT ? double( mem.L( sp ) ) : rms_double( mem.L( sp ), mem.H( sp ) );
				const double	b = t2 == RMS_T_INT ? double( mem.L( top ) ) : rms_double( mem.L( top ), mem.H( top ) );
				const double	d = op == RMS_OP_ADD ? a + b : op == RMS_OP_SUB ? a - b : op == RMS_OP_MUL ? a * b : a / b;
				if( t1 == RMS_T_INT )
					mem.L( sp ) = int( d );		// the int operand keeps its type
				else{
					int32_t	lo, hi;
					rms_words( d, &lo, &hi );
					mem.L( sp ) = lo;
					mem.H( sp ) = hi;
				}
			}else if( rms_is_string( t1 ) && rms_is_string( t2 ) && op == RMS_OP_ADD ){
				if( !text )
					RMS_STOP( RMS_STOP_STRCAT, 0, 0, 0 );
				const int	n1 = mem.H( sp ), n2 = mem.H( top );
				if( n1 < 0 || n2 < 0 || n1 + n2 > mem.heap_cap - hp )
					RMS_STOP( RMS_STOP_HEAP, n1 + n2, mem.heap_cap, hp );
				for( int i = 0; i < n1; i++ )
					mem.HB( hp + i ) = rms_char_t<TEXT>( m, bases, mem, t1, mem.L( sp ), i );
				for( int i = 0; i < n2; i++ )
					mem.HB( hp + n1 + i ) = rms_char_t<TEXT>( m, bases, mem, t2, mem.L( top ), i );
				mem.T( sp ) = RMS_T_HSTR;
				mem.L( sp ) = hp;
				mem.H( sp ) = n1 + n2;
				hp += n1 + n2;
			}
			else
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			break;
		}
		case RMS_OP_NEG :
			if( mem.T( sp ) == RMS_T_INT )
				mem.L( sp ) = int32_t( 0u - uint32_t( mem.L( sp ) ) );
			else if( mem.T( sp ) == RMS_T_FLOAT ){
				int32_t	lo, hi;
				rms_words( -rms_double( mem.L( sp ), mem.H( sp ) ), &lo, &hi );
				mem.L( sp ) = lo;
				mem.H( sp ) = hi;
			}else
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			break;
		case RMS_OP_I_PP : case RMS_OP_PP_I : case RMS_OP_I_MM : case RMS_OP_MM_I : {	// do_incr
			if( mem.T( sp ) != RMS_T_IDENT )
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			const int	v = mem.L( sp );
			if( mem.VT( v ) == RMS_T_UNDEF )
				RMS_STOP( RMS_STOP_UNDEF_VAR, v, 0, 0 );
			if( mem.VT( v ) != RMS_T_INT )
				RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
			const int32_t	old = mem.VL( v );
			const int32_t	now = int32_t( uint32_t( old ) + ( ip.op == RMS_OP_I_PP || ip.op == RMS_OP_PP_I ? 1u : ~0u ) );
			mem.VL( v ) = now;
			mem.L( sp ) = ip.op == RMS_OP_I_PP || ip.op == RMS_OP_I_MM ? old : now;	// (sic) the slot keeps its identifier type
			break;
		}
		case RMS_OP_FJP :
			if( sp < 0 )
				RMS_STOP( RMS_STOP_INTERNAL, 3, 0, 0 );
			if( !mem.L( sp ) )
				pc = ip.a;
			sp = mp = -1;
			break;
		case RMS_OP_JMP :
			pc = ip.a;
			break;
		case RMS_OP_STRF : {		// do_strf
			int	len = mem.L( sp ), pos = mem.L( sp - 1 );
			const int	index = mem.L( sp - 2 );
			if( index < 0 || index >= n_xd )
				RMS_STOP( RMS_STOP_STRF_NODESCR, index, 0, 0 );
			const int	row = xd[ index ], mlen = RMS_MLEN( row );
			if( pos == -1 )
				pos = 1;
			else if( pos < 0 )
				RMS_STOP( RMS_STOP_STRF_POS_NEG, pos, 0, 0 );
			else if( mlen == 0 )
				pos = 1;
			else if( pos > mlen )
				RMS_STOP( RMS_STOP_STRF_POS_BIG, pos, mlen, 0 );
			pos--;
			if( len == 0 )
				RMS_STOP( RMS_STOP_STRF_LEN, len, 0, 0 );
			else if( len == -1 )
				len = mlen - pos;
			else
				len = mlen - pos < len ? mlen - pos : len;
			if( len < 0 )
				len = 0;
			sp -= 2;
			mem.T( sp ) = RMS_T_BSTR;
			mem.L( sp ) = RMS_MOFF( row ) + pos;
			mem.H( sp ) = len;
			esp--;
			break;
		}
		case RMS_OP_SCL : {		// do_scl
			int	rt = RMS_T_INT, rl = 0, rh = 0;		// what the call returns to the mark
			switch( ip.a ){
			case RMS_SC_STRID : {		// strid
				const int	t = mem.T( sp ), stype = mem.L( sp - 1 );
				int	idx = -1;
				if( t == RMS_T_INT ){
					idx = mem.L( sp );
					if( idx < 1 || idx > n_xd )
						RMS_STOP( RMS_STOP_STRID_RANGE, idx, n_xd, 0 );
					idx--;
					if( stype != m->sym_se && rows[ xd[ idx ] ].type != stype )
						RMS_STOP( RMS_STOP_STRID_TYPE, stype, rows[ xd[ idx ] ].type, 0 );
				}else if( rms_is_string( t ) ){
					for( int s = 0; s < n_xd && idx < 0; s++ ){
						const RmsElem	&el = rows[ xd[ s ] ];
						if( el.tag_len < 0 || rms_strcmp_t<TEXT>( m, bases, mem, RMS_T_STRING, el.tag_off, el.tag_len, t, mem.L( sp ), mem.H( sp ) ) )
							continue;
						if( el.type == stype || ( el.type == m->sym_ss && stype == m->sym_se ) )
							idx = s;
					}
					if( idx < 0 )
						RMS_STOP( RMS_STOP_STRID_TAG, t, mem.L( sp ), mem.H( sp ) );
				}
				rl = idx;
				if( esp + 1 >= RMS_ESTK )
					RMS_STOP( RMS_STOP_ESTK, 0, 0, 0 );
				mem.E( ++esp ) = uint8_t( idx );
				break;
			}
			case RMS_SC_EFN :
			case RMS_SC_EFN2 : {		// do_efn
				const int	kind = ip.a == RMS_SC_EFN2 ? RMA_EFN_KIND_EFN2 : RMA_EFN_KIND_EFN;
				const int	idx = mem.L( sp - 5 ), idx2 = mem.L( sp - 2 );
				int	pos = mem.L( sp - 4 ), pos2 = mem.L( sp - 1 );
				if( idx < 0 || idx >= n_xd )
					RMS_STOP( RMS_STOP_XD, RMS_SC_EFN, idx + 1, n_xd );
				const int	mlen = RMS_MLEN( xd[ idx ] );
				if( pos == -1 )
					pos = 1;
				else if( pos <= 0 )
					RMS_STOP( RMS_STOP_EFN_POS1_NEG, pos, 0, 0 );
				else if( mlen == 0 )
					RMS_STOP( RMS_STOP_EFN_LEN1, 0, 0, 0 );
				else if( pos > mlen )
					RMS_STOP( RMS_STOP_EFN_POS1_BIG, pos, mlen, 0 );
				pos--;
				if( idx2 < 0 || idx2 >= n_xd )
					RMS_STOP( RMS_STOP_XD, RMS_SC_EFN, idx2 + 1, n_xd );
				if( idx >= idx2 )
					RMS_STOP( RMS_STOP_EFN_ORDER, idx2 + 1, idx + 1, 0 );
				const int	mlen2 = RMS_MLEN( xd[ idx2 ] );
				if( pos2 == -1 )
					pos2 = mlen2;
				else if( pos2 < 0 )
					RMS_STOP( RMS_STOP_EFN_POS2_NEG, pos2, 0, 0 );
				else if( mlen2 == 0 )
					RMS_STOP( RMS_STOP_EFN_LEN2, 0, 0, 0 );
				else if( pos > mlen2 )		// (sic) pos, not pos2
					RMS_STOP( RMS_STOP_EFN_POS2_BIG, pos2, mlen2, 0 );
				pos2--;
				// the energy is the record's word for this call site
				const rma_efn_site_t	*site = rms_efn( m );
				int	k = 0;
				for( ; k < m->n_efn; k++ ){
					const rma_efn_site_t	&s = site[ k ];
					const int	want2 = s.pos2 < 0 ? mlen2 - 1 : s.pos2;
					if( s.kind == kind && s.idx + m->x_off == idx && s.idx2 + m->x_off == idx2 && s.pos == pos && want2 == pos2 )
						break;
				}
				if( k == m->n_efn )
					RMS_STOP( RMS_STOP_EFN_NO_SITE, 0, 0, 0 );
				const float	rval = 0.01 * w[ m->efn_off + k ];
				rt = RMS_T_FLOAT;
				rms_words( double( rval ), &rl, &rh );
				break;
			}
			case RMS_SC_LENGTH :
				if( !rms_is_string( mem.T( sp ) ) )
					RMS_STOP( RMS_STOP_LENGTH_ARG, 0, 0, 0 );
				rl = mem.H( sp );
				break;
			case RMS_SC_LOC : {
				const int	idx = mem.L( sp - 2 ), pos = mem.L( sp - 1 );
				if( idx < 0 || idx >= n_xd )
					RMS_STOP( RMS_STOP_LOC_RANGE, idx + 1, n_xd, 0 );
				const int	mlen = RMS_MLEN( xd[ idx ] );
				if( pos == -1 )
					;
				else if( pos < 0 )
					RMS_STOP( RMS_STOP_LOC_POS_NEG, pos, 0, 0 );
				else if( mlen == 0 )
					RMS_STOP( RMS_STOP_LOC_LEN, mlen, 0, 0 );
				else if( pos > mlen )
					RMS_STOP( RMS_STOP_LOC_POS_BIG, pos, mlen, 0 );
				rl = RMS_MOFF( xd[ idx ] ) + 1;
				break;
			}
			case RMS_SC_MISMATCHES_1 :
			case RMS_SC_MISPAIRS : {
				const int	idx = mem.L( sp - 2 );
				if( idx < 0 || idx >= n_xd )
					RMS_STOP( RMS_STOP_XD, ip.a, idx + 1, n_xd );
				const int	row = xd[ idx ];
				// (a context's counts are never set: Strel's UNDEF)
				rl = row >= m->n_elems ? -1 : w[ RMA_HIT_HDR + 4 * row + ( ip.a == RMS_SC_MISPAIRS ? 2 : 3 ) ];
				break;
			}
			case RMS_SC_PAIRED : {
				const int	idx = mem.L( sp - 2 );
				int	pos = mem.L( sp - 1 ), len = mem.L( sp );
				if( idx < 0 || idx >= n_xd )
					RMS_STOP( RMS_STOP_XD, RMS_SC_PAIRED, idx + 1, n_xd );
				const RmsElem	&st = rows[ xd[ idx ] ];
				const int	mlen = RMS_MLEN( xd[ idx ] );
				if( pos < 1 || pos > mlen )
					RMS_STOP( RMS_STOP_PAIRED_POS, pos, mlen, 0 );
				pos--;
				if( len == 0 )
					RMS_STOP( RMS_STOP_PAIRED_LEN, len, 0, 0 );
				else if( len < 0 )
					len = mlen - pos;
				else
					len = mlen - pos < len ? mlen - pos : len;
				// paired()
				if( st.n_mates < 1 || st.n_mates > 3 )
					RMS_STOP( RMS_STOP_PAIRED_SS, 0, 0, 0 );
				const int	r1 = st.index < rows[ st.mates[ 0 ] ].index ? xd[ idx ] : st.mates[ 0 ];
				const RmsElem	&s1 = rows[ r1 ];
				if( s1.n_mates < 1 )
					RMS_STOP( RMS_STOP_INTERNAL, 4, 0, 0 );
				// (a duplex and a triplex read their first strand's pair set; a quad reads none)
				if( st.n_mates <= 2 && unsigned( s1.ps ) >= unsigned( m->n_ps ) )
					RMS_STOP( RMS_STOP_INTERNAL, 4, 0, 0 );
				const rma_pairset_t	*ps = rms_ps( m ) + ( st.n_mates <= 2 ? s1.ps : 0 );
				const int	p1 = RMS_MOFF( r1 ), p2 = RMS_MOFF( s1.mates[ 0 ] ) + mlen - 1;
				rl = 1;
				if( st.n_mates == 1 ){
					for( int i = 0; i < len && rl; i++ )
						rl = ( ps->mat2 >> ( rms_b2bc( bases( p1 + pos + i ) ) * 5 + rms_b2bc( bases( p2 - pos - i ) ) ) ) & 1;
				}else if( st.n_mates == 2 ){
					if( s1.n_mates < 2 )
						RMS_STOP( RMS_STOP_INTERNAL, 5, 0, 0 );
					const int	p3 = RMS_MOFF( s1.mates[ 1 ] );
					for( int i = 0; i < len && rl; i++ ){
						const int	ix = ( rms_b2bc( bases( p1 + pos + i ) ) * 5 + rms_b2bc( bases( p2 - pos - i ) ) ) * 5 +
							rms_b2bc( bases( p3 + pos + i ) );
						rl = ( ps->mat3[ ix >> 5 ] >> ( ix & 31 ) ) & 1;
					}
				}
				// (sic) a quad is paired whatever its bases
				break;
			}
			case RMS_SC_SUBSTR : {
				const int	t = mem.T( sp - 2 );
				if( !rms_is_string( t ) )
					RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
				const int	c_len = mem.H( sp - 2 ), pos = mem.L( sp - 1 );
				int	len = mem.L( sp );
				if( pos < 1 || pos > c_len )
					RMS_STOP( RMS_STOP_SUBSTR_POS, pos, c_len, 0 );
				if( len < 1 )
					RMS_STOP( RMS_STOP_SUBSTR_LEN, len, 0, 0 );
				len = c_len - pos + 1 < len ? c_len - pos + 1 : len;
				rt = t;
				rl = mem.L( sp - 2 ) + pos - 1;
				rh = len;
				break;
			}
			case RMS_SC_BITS : {		// do_bits
				if( !text )
					RMS_STOP( RMS_STOP_INTERNAL, 6, 0, 0 );
				const int	idx = mem.L( sp - 5 ), idx2 = mem.L( sp - 2 );
				int	pos = mem.L( sp - 4 ), pos2 = mem.L( sp - 1 );
				if( idx < 0 || idx >= n_xd )
					RMS_STOP( RMS_STOP_XD, RMS_SC_BITS, idx + 1, n_xd );
				const int	mlen = RMS_MLEN( xd[ idx ] );
				if( pos == -1 )
					pos = 1;
				else if( pos <= 0 )
					RMS_STOP( RMS_STOP_BITS_POS1_NEG, pos, 0, 0 );
				else if( mlen == 0 )
					RMS_STOP( RMS_STOP_BITS_LEN1, 0, 0, 0 );
				else if( pos > mlen )
					RMS_STOP( RMS_STOP_BITS_POS1_BIG, pos, mlen, 0 );
				pos--;
				if( idx2 < 0 || idx2 >= n_xd )
					RMS_STOP( RMS_STOP_XD, RMS_SC_BITS, idx2 + 1, n_xd );
				if( idx >= idx2 )
					RMS_STOP( RMS_STOP_BITS_ORDER, idx + 1, idx2 + 1, 0 );	// (sic) the other way round than efn's
				const int	mlen2 = RMS_MLEN( xd[ idx2 ] );
				if( pos2 == -1 )
					pos2 = mlen2;
				else if( pos2 < 0 )
					RMS_STOP( RMS_STOP_BITS_POS2_NEG, pos2, 0, 0 );
				else if( mlen2 == 0 )
					RMS_STOP( RMS_STOP_BITS_LEN2, 0, 0, 0 );
				else if( pos2 > mlen2 )
					RMS_STOP( RMS_STOP_BITS_POS2_BIG, pos2, mlen2, 0 );
				pos2--;
				const int	start = RMS_MOFF( xd[ idx ] ) + pos, stop = RMS_MOFF( xd[ idx2 ] ) + pos2, len = stop - start + 1;
				if( len > m->bits_L || ( len > 0 && tx.bits_tab == nullptr ) )
					RMS_STOP( RMS_STOP_BITS_SPAN, len, m->bits_L, 0 );
				// bvec[] in bindex[]'s order: the counts by letter, 16 bits each, and the letters in the order they first occur
				uint64_t	counts = 0;
				unsigned	seen = 0, order = 0;
				int	bn = 0;
				for( int i = start; i <= stop; i++ ){
					const int	bc = rms_b2bc( bases( i ) );
					if( bc != RMA_BC_N ){
						if( !( ( seen >> bc ) & 1 ) ){
							seen |= 1u << bc;
							order |= unsigned( bc ) << ( 2 * bn++ );
						}
						counts += uint64_t( 1 ) << ( 16 * bc );
					}
				}
#ifdef RMS_ON_BITS
				RMS_ON_BITS( bn, len );		// (a host checker counts the windows and their distinct letters)
#endif
				double	bits = 0.0;
				for( int i = 0; i < bn; i++ ){
					const int	b = int( ( counts >> ( 16 * ( ( order >> ( 2 * i ) ) & 3 ) ) ) & 0xffff );
					bits += b * tx.bits_tab[ ( len - 1 ) * len / 2 + b - 1 ];
				}
				bits /= -len;
				const float	rval = float( bits );
				rt = RMS_T_FLOAT;
				rms_words( double( rval ), &rl, &rh );
				break;
			}
			case RMS_SC_SPRINTF : {		// do_sprintf
				if( !text )
					RMS_STOP( RMS_STOP_INTERNAL, 6, 0, 0 );
				const int	n_args = sp - mp;
				if( mp < 0 || n_args < 1 || !rms_is_string( mem.T( mp + 1 ) ) )
					RMS_STOP( RMS_STOP_SPF_FIRST, 0, 0, 0 );
				const RmsStr<TEXT, Mem, Bases>	f{ m, bases, mem, mem.T( mp + 1 ), mem.L( mp + 1 ) };
				const int	fn = mem.H( mp + 1 );
				RmsSink	o{ mem.heap, Mem::stride, hp, mem.heap_cap, 0 };
				int	c_arg = 0, fp = 0;
				for( ; ; ){
					int	pp = fp;
					while( pp < fn && f( pp ) != '%' )
						pp++;
					if( pp >= fn )
						break;
					for( int i = fp; i < pp; i++ )
						o.put( f( i ) );
					int	epp = pp + 1;
					while( epp < fn && !rms_fmt_is_conv( f( epp ) ) )
						epp++;
					if( epp >= fn )
						RMS_STOP( RMS_STOP_SPF_BAD, f.type, f.off + pp, fn - pp );
					const int	type = f( epp );
					for( int i = pp; i <= epp; i++ )
						if( f( i ) == '*' || f( i ) == '$' )
							RMS_STOP( RMS_STOP_SPF_STAR, 0, 0, 0 );
					const int	r_arg = c_arg + 1;
					if( r_arg >= n_args )
						RMS_STOP( RMS_STOP_SPF_NO_ARG, r_arg, 0, 0 );
					const int	v = mp + r_arg + 1, vt = mem.T( v );
					c_arg++;
					RmsSpec	spec;
					const int	plain = rms_fmt_parse( f, pp + 1, epp, &spec );
					switch( type ){
					case 'e' : case 'E' : case 'f' : case 'g' : case 'G' : {
						if( vt != RMS_T_FLOAT )
							RMS_STOP( RMS_STOP_SPF_NEED_FLOAT, type, 0, 0 );
						if( type != 'f' )
							RMS_STOP( RMS_STOP_SPF_EG, type, 0, 0 );
						if( !plain )
							RMS_STOP( RMS_STOP_SPF_MODIFIER, type, 0, 0 );
						const int	rc = rms_fmt_f( o, spec, rms_double( mem.L( v ), mem.H( v ) ) );
						if( rc == RMS_FMT_PREC )
							RMS_STOP( RMS_STOP_SPF_PREC, spec.prec, 0, 0 );
						if( rc != RMS_FMT_OK )
							RMS_STOP( RMS_STOP_SPF_RANGE, 0, 0, 0 );
						break;
					}
					case 'd' : case 'i' : case 'o' : case 'u' : case 'x' : case 'X' :
						if( vt != RMS_T_INT )
							RMS_STOP( RMS_STOP_SPF_NEED_INT, type, 0, 0 );
						if( !plain )
							RMS_STOP( RMS_STOP_SPF_MODIFIER, type, 0, 0 );
						rms_fmt_int( o, spec, static_cast<unsigned char>( type ), mem.L( v ) );
						break;
					case 's' :
						if( !rms_is_string( vt ) )
							RMS_STOP( RMS_STOP_SPF_NEED_STRING, type, 0, 0 );
						if( !plain )
							RMS_STOP( RMS_STOP_SPF_MODIFIER, type, 0, 0 );
						rms_fmt_str( o, spec, RmsStr<TEXT, Mem, Bases>{ m, bases, mem, vt, mem.L( v ) }, mem.H( v ) );
						break;
					case 'n' :		// (the argument's slot is set to 0, nothing is written)
						if( vt == RMS_T_INT )
							mem.L( v ) = 0;
						else if( vt == RMS_T_FLOAT )
							mem.L( v ) = mem.H( v ) = 0;
						else
							RMS_STOP( RMS_STOP_SPF_NEED_INT, type, 0, 0 );
						break;
					case '%' :		// (sic) it has taken an argument's place
						o.put( '%' );
						break;
					default :
						RMS_STOP( RMS_STOP_SPF_UNSUPPORTED, type, 0, 0 );
					}
					fp = epp + 1;
				}
				for( int i = fp; i < fn; i++ )
					o.put( f( i ) );
				if( o.n > mem.heap_cap - hp )
					RMS_STOP( RMS_STOP_HEAP, o.n, mem.heap_cap, hp );
				rt = RMS_T_HSTR;
				rl = hp;
				rh = o.n;
				hp += o.n;
				break;
			}
			case RMS_SC_MISMATCHES_2 : {	// (the host takes both for strings unasked)
				if( !MATCH || !( m->flags & RMS_IMG_MATCH ) || unsigned( ip.len ) >= unsigned( m->n_expr ) )
					RMS_STOP( RMS_STOP_INTERNAL, 6, 0, 0 );
				if( sp - 1 <= mp || !rms_is_string( mem.T( sp - 1 ) ) )
					RMS_STOP( RMS_STOP_TYPE, 0, 0, 0 );
				const RmsMatchExpr	ex = rms_match_expr( m )[ ip.len ];
				int	n_mm = 0;
				if( ex.n_ops >= 0 ){
					const RmsMatchText<TEXT, Mem, Bases>	text{ m, bases, mem, mem.T( sp - 1 ), mem.L( sp - 1 ), mem.H( sp - 1 ) };
					if( rmq_mm_step( rms_match_ops( m ) + ex.first, ex.n_ops, text, ex.anchored != 0, 20 * ex.pat_len, &n_mm, budget, &steps ) < 0 )
						RMS_STOP( RMS_STOP_BUDGET, budget, 0, 0 );
				}
				rl = n_mm;
				break;
			}
			default :		// no image holds it
				RMS_STOP( RMS_STOP_INTERNAL, 6, 0, 0 );
			}
			if( mp < 0 )
				RMS_STOP( RMS_STOP_INTERNAL, 7, 0, 0 );
			sp = mp;
			mp = mem.L( mp );
			mem.T( sp ) = rt;
			mem.L( sp ) = rl;
			mem.H( sp ) = rh;
			break;
		}
		default :		// HALT, HOLD, RLSE, FCL: no image holds them
			RMS_STOP( RMS_STOP_INTERNAL, 8, 0, 0 );
		}
	}
accept:
	// what print_match() reads of SCORE
	{
		const int	t = m->v_score >= 0 ? mem.VT( m->v_score ) : RMS_T_UNDEF;
		if( rms_is_string( t ) && !( TEXT && tx.row != nullptr ) )
			RMS_STOP( RMS_STOP_SCORE_STRING, 0, 0, 0 );
		if( t == RMS_T_INT ){
			r->kind = RMS_KIND_INT;
			r->score = double( mem.VL( m->v_score ) );
		}else if( t == RMS_T_FLOAT ){
			r->kind = RMS_KIND_FLOAT;
			r->score = rms_double( mem.VL( m->v_score ), mem.VH( m->v_score ) );
		}else if( rms_is_string( t ) )
			r->kind = RMS_KIND_STRING;
		if( TEXT && tx.row != nullptr ){
			// the score column of HitPrinter::print: %8d, %8s, %8.3lf (of 0.0 where SCORE is none of these)
			RmsSink	o{ tx.row, 1, 0, tx.row_cap, 0 };
			if( t == RMS_T_INT )
				rms_fmt_int( o, RmsSpec{ 0, 8, -1 }, 'd', mem.VL( m->v_score ) );
			else if( rms_is_string( t ) )
				rms_fmt_str( o, RmsSpec{ 0, 8, -1 }, RmsStr<TEXT, Mem, Bases>{ m, bases, mem, t, mem.VL( m->v_score ) }, mem.VH( m->v_score ) );
			else if( rms_fmt_f( o, RmsSpec{ 0, 8, 3 }, r->score ) != RMS_FMT_OK ){
				r->kind = RMS_KIND_NONE;
				r->score = 0.0;
				RMS_STOP( RMS_STOP_TEXT_RANGE, 0, 0, 0 );
			}
			if( o.n > tx.row_cap ){
				r->kind = RMS_KIND_NONE;
				r->score = 0.0;
				RMS_STOP( RMS_STOP_TEXT_ROOM, o.n, tx.row_cap, 0 );
			}
			r->text_len = o.n;
		}
		r->outcome = RMS_ACCEPT;
	}
#undef RMS_STOP
#undef RMS_MLEN
#undef RMS_MOFF
}

// the rule of an image opened without RMS_IMG_TEXT, and of a call that delivers numbers
template< class Mem, class Bases >
RMD_FN void rms_run( const RmsImage *m, const int32_t *w, int slen, const Bases &bases, const Mem &mem, int budget, RmsResult *r )
{
	rms_run_t<false>( m, w, slen, bases, mem, budget, r, RmsText() );
}
// with the heap (RmsMem::heap), the table of bits() and, where tx.row is set, the score column
template< class Mem, class Bases >
RMD_FN void rms_run( const RmsImage *m, const int32_t *w, int slen, const Bases &bases, const Mem &mem, int budget, RmsResult *r, const RmsText &tx )
{
	rms_run_t<true>( m, w, slen, bases, mem, budget, r, tx );
}
