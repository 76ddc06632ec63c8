// rm_seqcheck.h -- the seq= expressions the scan tests loosely (rma_regex_t::loose: back references, \< \>, letters that
// are not acgt with iupac = 0), applied to the element text of a hit record: what Replayer::one_hit does with re_step() /
// re_mm_step() of rm_regex.cpp before it counts a candidate, as one rule for the host and for rma_seqcheck_kernel
// (rm_seqcheck_dev.hip).  A record that passes is a candidate of the reference's; one that fails is none.
//
// The image is one block of bytes: a header (RmqImage) with one RmqExpr per loose element, in the order of the elements,
// and behind it the ops of all expressions (RmqOp: ReOp of rm_regex.h, flattened).  The first `bytes` bytes are all the
// rule reads; a kernel copies them to LDS.
//
// The matcher is advance() of rm_regex.cpp (regexp.c:426-664) without its recursion.  advance() calls itself from one
// place, the longest-first loop of an op that repeats (a star, a \{lo,hi\}, a starred back reference), always with
// ip + 1: along a chain of calls ip grows strictly, so an op is on the chain at most once and one frame per repeating op
// of the expression is all the stack there can be.  A frame is what that loop keeps: the op, the position lp it tries
// next, the floor cur below which it gives up, and the step ct it goes down by (1 for a character, the group's length
// for a back reference, where 0 means one try).  A failure anywhere resumes the innermost frame one step down, as the
// return of the nested call does.  bra[] and ket[] are written when \( and \) are passed and never restored, as in the
// reference.  The end of the string is the byte 0 at position len: the text is read through an accessor inside
// [off, off + len) only.
//
// Limits (a descriptor beyond them is refused when the image is made):
//   RMQ_MAX_EXPR   expressions (loose elements)
//   RMQ_MAX_OPS    ops of one expression
//   RMQ_LDS_BYTES  the image, two letter tables and one wave's planes (rm_seqcheck_dev.h) must fit this much LDS; the
//                  planes are 18 words for bra[] and ket[] and RMQ_FRAME_WORDS per frame, 64 lanes each
#pragma once
#include <cstdint>
#include "rnamotif_amd_program.h"

#if defined( __HIPCC__ )
#define RMQ_FN	__host__ __device__ inline
#else
#define RMQ_FN	inline
#endif

enum {
	RMQ_MAX_EXPR = 20, RMQ_MAX_OPS = 255, RMQ_LDS_BYTES = 64 * 1024, RMQ_LDS_TABLES = 512, RMQ_MAX_WAVES = 4,
	RMQ_NBRA = 9, RMQ_FRAME_WORDS = 4, RMQ_FIXED_SLOTS = 2 * RMQ_NBRA
};
#define RMQ_MAGIC	0x524d5131u	/* "RMQ1" */
#define RMQ_DEFAULT_BUDGET	( 1 << 20 )

// ReKind and ReRep of rm_regex.h, by value (rm_seqcheck.cpp asserts it)
enum { RMQ_CHR, RMQ_DOT, RMQ_CCL, RMQ_NCCL, RMQ_DOL, RMQ_BRA, RMQ_KET, RMQ_BACK, RMQ_BRC, RMQ_LET };
enum { RMQ_ONE, RMQ_STAR, RMQ_RANGE };

struct RmqOp {
	uint8_t	kind, rep, c, lo, hi, pad[ 3 ];
	uint32_t	set[ 4 ];	// RMQ_CCL / RMQ_NCCL: 128-bit membership
};

struct RmqExpr {
	int32_t	elem;		// the element's index
	int32_t	anchored;	// *seq == '^'
	int32_t	mismatch;	// the element's limit; > 0: mm_step
	int32_t	first, n_ops;	// its ops among the image's
	int32_t	pad;
};

struct RmqImage {
	uint32_t	magic;
	int32_t	bytes;
	int32_t	n_expr, n_ops;
	int32_t	frames;		// frames of the stack: the most repeating ops of one expression
	int32_t	stride;		// of the hit record
	RmqExpr	expr[ RMQ_MAX_EXPR ];
	// RmqOp ops[ n_ops ] behind it
};
static_assert( sizeof( RmqOp ) == 24 && sizeof( RmqExpr ) == 24 && sizeof( RmqImage ) % 8 == 0, "the image is packed" );

RMQ_FN const RmqOp *rmq_ops( const RmqImage *m ) { return reinterpret_cast<const RmqOp *>( m + 1 ); }

// words (of one lane) and bytes (of a wave) of the planes
constexpr int rmq_slots( int frames ) { return RMQ_FIXED_SLOTS + RMQ_FRAME_WORDS * frames; }
constexpr int rmq_wave_bytes( int frames ) { return rmq_slots( frames ) * 64 * 4; }
// the frames one wave can have next to an image of this size (< 0: the image alone is too large)
constexpr int rmq_frames_cap( int image_bytes )
{
	return RMQ_LDS_BYTES - RMQ_LDS_TABLES - image_bytes < RMQ_FIXED_SLOTS * 64 * 4 ? -1 :
		( ( RMQ_LDS_BYTES - RMQ_LDS_TABLES - image_bytes ) / ( 64 * 4 ) - RMQ_FIXED_SLOTS ) / RMQ_FRAME_WORDS;
}

enum { RMQ_KEEP = 0, RMQ_DROP = 1, RMQ_STOPPED = 2 };

struct RmqResult {
	int32_t	outcome;	// RMQ_*
	int32_t	elem;		// RMQ_DROP, RMQ_STOPPED: the element whose expression failed or ran out of steps
	int32_t	steps;		// ops visited (RMQ_STOPPED: budget + 1)
};

// A lane's runtime-indexed state: slot k at base[ k * STRIDE ].  Slots 0-8 bra[], 9-17 ket[], then the frames (a push
// beyond them, which the image's count of repeating ops rules out, stops the record like the budget).
template<int STRIDE>
struct RmqMem {
	int32_t	*base;
	int	frames;
	RMQ_FN int32_t	&at( int k ) const { return base[ k * STRIDE ]; }
	RMQ_FN int32_t	&bra( int g ) const { return at( g ); }
	RMQ_FN int32_t	&ket( int g ) const { return at( RMQ_NBRA + g ); }
	RMQ_FN int32_t	&frame( int f, int j ) const { return at( RMQ_FIXED_SLOTS + RMQ_FRAME_WORDS * f + j ); }
};
enum { RMQ_F_IP, RMQ_F_LP, RMQ_F_CUR, RMQ_F_CT };

RMQ_FN bool rmq_has( const RmqOp &op, int ch ) { return ( op.set[ ch >> 5 ] >> ( ch & 31 ) ) & 1u; }
// isalpha() || '_' || isdigit() of the C locale
RMQ_FN bool rmq_word( int ch )
{
	return ( ch >= 'a' && ch <= 'z' ) || ( ch >= 'A' && ch <= 'Z' ) || ch == '_' || ( ch >= '0' && ch <= '9' );
}

// one element's text: byte k of the NUL terminated copy chk_seq() makes of it
template<class Bases>
struct RmqText {
	const Bases	&bases;
	int	off, len;
	RMQ_FN int	operator()( int k ) const { return k < len ? int( bases( off + k ) ) : 0; }
};

RMQ_FN bool rmq_one( const RmqOp &op, int ch )
{
	switch( op.kind ){
	case RMQ_CHR :	return ch == op.c;
	case RMQ_DOT :	return ch != 0;
	case RMQ_CCL :	return ( ch & 0200 ) == 0 && rmq_has( op, ch );
	case RMQ_NCCL :	return !( ( ch & 0200 ) == 0 && rmq_has( op, ch ) );
	default :	return false;
	}
}

// strncmp( bb, lp, ct ) == 0 on the text
template<class Text>
RMQ_FN bool rmq_same( const Text &text, int bb, int lp, int ct )
{
	for( int k = 0; k < ct; k++ ){
		const int	a = text( bb + k );
		if( a != text( lp + k ) )
			return false;
		if( a == 0 )
			break;
	}
	return true;
}

// advance( lp, 0 ): 1 a match, 0 none, -1 out of steps
template<class Text, class Mem>
RMQ_FN int rmq_advance( const RmqOp *ops, int n_ops, const Text &text, const Mem &mem, int lp, int budget, int *steps )
{
	int	ip = 0, sp = 0;
	for( ; ; ){
		// forwards, until the end of the expression or an op that fails
		bool	failed = false;
		while( !failed ){
			if( ++*steps > budget )
				return -1;
			if( ip == n_ops )
				return 1;
			const RmqOp	&op = ops[ ip ];
			switch( op.kind ){
			case RMQ_DOL :
				failed = text( lp ) != 0;
				break;
			case RMQ_BRA :
				mem.bra( op.c ) = lp;
				break;
			case RMQ_KET :
				mem.ket( op.c ) = lp;
				break;
			case RMQ_BRC :
				if( lp != 0 )
					failed = !( rmq_word( text( lp ) ) && !rmq_word( text( lp - 1 ) ) );
				break;
			case RMQ_LET :
				failed = rmq_word( text( lp ) );
				break;
			case RMQ_BACK : {
				const int	bb = mem.bra( op.c ), ct = mem.ket( op.c ) - bb;
				if( op.rep == RMQ_ONE ){
					if( rmq_same( text, bb, lp, ct ) )
						lp += ct;
					else
						failed = true;
					break;
				}
				if( sp >= mem.frames )
					return -1;
				const int	cur = lp;
				while( ct > 0 && rmq_same( text, bb, lp, ct ) )
					lp += ct;
				mem.frame( sp, RMQ_F_IP ) = ip;
				mem.frame( sp, RMQ_F_LP ) = lp;
				mem.frame( sp, RMQ_F_CUR ) = cur;
				mem.frame( sp, RMQ_F_CT ) = ct;
				sp++;
				break;
			}
			default :	// the single character ops
				if( op.rep == RMQ_ONE ){
					if( rmq_one( op, text( lp ) ) )
						lp++;
					else
						failed = true;
					break;
				}else{
					int	lo = 0, extra = 0x7fffffff;
					if( op.rep == RMQ_RANGE ){
						lo = op.lo;
						extra = op.hi == 255 ? 20000 : op.hi - op.lo;
					}
					for( ; lo > 0 && !failed; lo-- ){
						if( rmq_one( op, text( lp ) ) )
							lp++;
						else
							failed = true;
					}
					if( failed )
						break;
					if( sp >= mem.frames )
						return -1;
					const int	cur = lp;
					for( ; extra > 0 && rmq_one( op, text( lp ) ); extra-- )
						lp++;
					mem.frame( sp, RMQ_F_IP ) = ip;		// longest first, regexp.c:608-641
					mem.frame( sp, RMQ_F_LP ) = lp;
					mem.frame( sp, RMQ_F_CUR ) = cur;
					mem.frame( sp, RMQ_F_CT ) = 1;
					sp++;
				}
				break;
			}
			ip++;
		}
		// backwards: the innermost loop that has a shorter try left
		for( ; ; ){
			if( sp == 0 )
				return 0;
			const int	ct = mem.frame( sp - 1, RMQ_F_CT );
			const int	nlp = mem.frame( sp - 1, RMQ_F_LP ) - ct;
			if( ct == 0 || nlp < mem.frame( sp - 1, RMQ_F_CUR ) ){
				sp--;
				continue;
			}
			mem.frame( sp - 1, RMQ_F_LP ) = nlp;
			lp = nlp;
			ip = mem.frame( sp - 1, RMQ_F_IP ) + 1;
			break;
		}
	}
}

// step(): 1, 0 or -1 as rmq_advance
template<class Text, class Mem>
RMQ_FN int rmq_step( const RmqOp *ops, int n_ops, const Text &text, const Mem &mem, bool anchored, int budget, int *steps )
{
	if( anchored )
		return rmq_advance( ops, n_ops, text, mem, 0, budget, steps );
	int	p = 0;
	do{
		const int	r = rmq_advance( ops, n_ops, text, mem, p, budget, steps );
		if( r != 0 )
			return r;
	}while( text( p++ ) != 0 );
	return 0;
}

// mm_advance, mm_regexp.c:369-469, as rm_regex.cpp has it
template<class Text>
RMQ_FN int rmq_mm_advance( const RmqOp *ops, int n_ops, const Text &text, int lp, int l_mm, int *n_mm, int budget, int *steps )
{
	*n_mm = 0;
	for( int ip = 0; ip < n_ops; ip++ ){
		if( ++*steps > budget )
			return -1;
		const RmqOp	&op = ops[ ip ];
		int	reps = 1;
		if( op.rep == RMQ_RANGE )
			reps = op.lo;
		else if( op.rep == RMQ_STAR )
			continue;
		switch( op.kind ){
		case RMQ_CHR :
			for( ; reps > 0; reps-- ){
				const int	ch = text( lp++ );
				if( ch != op.c ){
					if( ch == 0 )
						return 0;
					if( ++*n_mm > l_mm )
						return 0;
				}
			}
			break;
		case RMQ_DOT :
			for( ; reps > 0; reps-- ){
				if( text( lp++ ) == 0 )
					return 0;
			}
			break;
		case RMQ_DOL :
			if( text( lp ) != 0 )
				return 0;
			break;
		case RMQ_CCL :
		case RMQ_NCCL : {
			const bool	neg = op.kind == RMQ_NCCL;
			for( ; reps > 0; reps-- ){
				const int	ch = text( lp++ );
				if( ch == 0 )
					return 0;
				const bool	in = ( ch & 0200 ) == 0 && rmq_has( op, ch );
				if( in == neg ){
					if( ++*n_mm > l_mm )
						return 0;
				}
			}
			break;
		}
		default :
			break;
		}
	}
	return 1;
}

// mm_step(): *n_mm as the last attempt leaves it
template<class Text>
RMQ_FN int rmq_mm_step( const RmqOp *ops, int n_ops, const Text &text, bool anchored, int l_mm, int *n_mm, int budget, int *steps )
{
	if( anchored )
		return rmq_mm_advance( ops, n_ops, text, 0, l_mm, n_mm, budget, steps );
	int	p = 0;
	do{
		const int	r = rmq_mm_advance( ops, n_ops, text, p, l_mm, n_mm, budget, steps );
		if( r != 0 )
			return r;
	}while( text( p++ ) != 0 );
	return 0;
}

// One record, in one_hit's order over the loose elements.  w: the record (checked: every element inside its entry);
// bases: position on the hit's strand -> letter; fixed: the fixed row (the input row's words already in it) or null --
// word RMA_HIT_HDR + 4 * e + 3 of an element with a mismatch limit becomes mm_step's n_mm when the record is kept, and
// is the input's again when it is not.
template<class Bases, class Mem>
RMQ_FN void rmq_run( const RmqImage *m, const int32_t *w, const Bases &bases, const Mem &mem, int budget, int32_t *fixed, RmqResult *r )
{
	const RmqOp	*ops = rmq_ops( m );
	r->outcome = RMQ_KEEP;
	r->elem = -1;
	r->steps = 0;
	int	x = 0;
	for( ; x < m->n_expr; x++ ){
		const RmqExpr	&ex = m->expr[ x ];
		const int	k = RMA_HIT_HDR + 4 * ex.elem;
		const RmqText<Bases>	text{ bases, w[ k ], w[ k + 1 ] };
		int	ok;
		if( ex.mismatch > 0 ){
			int	n_mm = 0;
			ok = rmq_mm_step( ops + ex.first, ex.n_ops, text, ex.anchored != 0, ex.mismatch, &n_mm, budget, &r->steps );
			if( fixed != nullptr )
				fixed[ k + 3 ] = n_mm;
		}else
			ok = rmq_step( ops + ex.first, ex.n_ops, text, mem, ex.anchored != 0, budget, &r->steps );
		if( ok != 1 ){
			r->outcome = ok == 0 ? RMQ_DROP : RMQ_STOPPED;
			r->elem = ex.elem;
			break;
		}
	}
	if( r->outcome != RMQ_KEEP && fixed != nullptr )
		for( int y = 0; y <= x; y++ )
			if( m->expr[ y ].mismatch > 0 )
				fixed[ RMA_HIT_HDR + 4 * m->expr[ y ].elem + 3 ] = w[ RMA_HIT_HDR + 4 * m->expr[ y ].elem + 3 ];
}

#ifndef RMQ_POD_ONLY
// ---- the host's half (rm_seqcheck.cpp)
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "rm_regex.h"

namespace rma {

struct Descriptor;

static_assert( int( RMQ_CHR ) == RE_CHR && int( RMQ_DOT ) == RE_DOT && int( RMQ_CCL ) == RE_CCL && int( RMQ_NCCL ) == RE_NCCL && int( RMQ_DOL ) == RE_DOL &&
	int( RMQ_BRA ) == RE_BRA && int( RMQ_KET ) == RE_KET && int( RMQ_BACK ) == RE_BACK && int( RMQ_BRC ) == RE_BRC && int( RMQ_LET ) == RE_LET,
	"the rule's op kinds are RE_*" );
static_assert( int( RMQ_ONE ) == REP_ONE && int( RMQ_STAR ) == REP_STAR && int( RMQ_RANGE ) == REP_RANGE, "the rule's repeats are REP_*" );

// The ops of a compiled expression, flattened, behind *ops; *repeats: how many of them repeat (the frames its matcher
// needs).  false: a group number beyond 9.  (seqcheck_image_make and score_image_make_flags, rm_score_image.cpp, both
// make their ops here; in the header, so that a checker built from the front end alone has it.)
inline bool rmq_flatten( const ReProg &re, std::vector<RmqOp> *ops, int *repeats )
{
	*repeats = 0;
	for( const ReOp &op : re.ops ){
		RmqOp	o;
		memset( &o, 0, sizeof( o ) );
		o.kind = op.kind;
		o.rep = op.rep;
		o.c = op.c;
		o.lo = op.lo;
		o.hi = op.hi;
		memcpy( o.set, op.set, sizeof( o.set ) );	// (little endian: bit ch of the 128 is bit ch & 31 of word ch >> 5)
		if( ( op.kind == RE_BRA || op.kind == RE_KET || op.kind == RE_BACK ) && op.c >= RMQ_NBRA )
			return false;
		if( op.rep != REP_ONE )
			++*repeats;
		ops->push_back( o );
	}
	return true;
}

struct SeqImage {
	std::vector<uint64_t>	blob;			// the image, 8-byte aligned
	const RmqImage	*image() const { return reinterpret_cast<const RmqImage *>( blob.data() ); }
	std::unique_ptr<rma_program_t>	prog;		// the descriptor's program: a scanner's must be the same, byte for byte
	uint64_t	serial = 0;			// of this image among all that were made (a scanner keeps the last one's on its device)
};

// The image of d's loose seq= expressions (none: an image of no expressions).  Returns "" or, with no image made, why not.
std::string	seqcheck_image_make( const Descriptor &d, const rma_program_t &prog, SeqImage *out );

}	// namespace rma

struct rma_seqcheck {
	rma::SeqImage	img;
};
#endif
