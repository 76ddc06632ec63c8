// rm_score_image.h -- the MAIN program of a descriptor's score section as a position-independent POD image, for the
// rule of rm_score_core.h: what ScoreVM (rm_score.h) keeps in Inst, Ident, Strel and PairSet objects, as indices.
//
// The image is one block of bytes: a header (RmsImage) and behind it, at the byte offsets the header names,
//   the instructions      RmsInst: op (OP_* of rm_score.h), operand kind, int / index of a double / slice of the pool
//   the doubles           the float constants of LDC
//   the variables         RmsVar: type and value after the parms section and BEGIN -- only those MAIN names, and SCORE
//   rm_xdescr             per entry the index of its row in the element table
//   the element table     RmsElem: rows 0 .. n_elems - 1 are rm_descr[], row n_elems the left context, n_elems + 1 the right
//   the pair sets         rma_pairset_t: the constants of LDC and the sets paired() reads
//   the energy call sites rma_efn_site_t, in the order of the record's energy words
//   the string pool       the bytes of string constants, of the strings variables hold after BEGIN, and of tags
//   the expressions       only in an image with RMS_IMG_MATCH whose MAIN has a =~, a !~ or a mismatches( string, pattern ):
//                         RmsMatch behind the pool -- per expression its anchor, its ops and its pattern's length, then the
//                         ops of all of them (RmqOp, rm_seqcheck.h); MAT's `a` and the builtin's `len` are the index
// The first `bytes` bytes are all the rule reads; a kernel copies them to LDS.  File and line of every instruction and
// the names of the variables stay on the host (rm_score_image.cpp: they are needed for the words of a stop only).
//
// Limits (a program beyond them is refused when the image is made; of the score sections under tests/golden that are
// not refused for another reason the longest, ire.descr, has 187 instructions, none names more than 5 variables,
// reaches a stack deeper than 9 slots or makes an image of more than 2584 bytes):
//   RMS_MAX_INST   instructions of MAIN
//   RMS_MAX_POOL   bytes of strings
//   RMS_MAX_VARS   variables MAIN names
//   RMS_MAX_STACK  slots of the operand stack (the deepest stack MAIN can reach, plus RMS_STACK_MARGIN)
//   RMS_MAX_PS     pair sets
//   RMS_LDS_BYTES  the image, two letter tables and one wave's planes (rm_score_dev.h) must fit this much LDS
//   RMS_MAX_EXPR   expressions (a =~, !~ or mismatches( string, pattern ) each has its own); one expression has at most
//                  RMQ_MAX_OPS ops, as in rm_seqcheck.h
#pragma once
#include <cstdint>
#include "rnamotif_amd_program.h"
#ifdef RMS_POD_ONLY
#ifndef RMQ_POD_ONLY
#define RMQ_POD_ONLY
#endif
#endif
#include "rm_seqcheck.h"

enum {
	RMS_MAX_INST = 4096, RMS_MAX_POOL = 8192, RMS_MAX_VARS = 64, RMS_MAX_STACK = 64, RMS_MAX_PS = 64,
	RMS_STACK_MARGIN = 2, RMS_ESTK = 20, RMS_LDS_BYTES = 64 * 1024, RMS_LDS_TABLES = 512,
	RMS_MAX_EXPR = 32
};
#define RMS_MAGIC	0x524d5331u	/* "RMS1" */
#define RMS_DEFAULT_BUDGET	( 1 << 20 )

// operand kinds
enum { RMS_K_NONE, RMS_K_INT, RMS_K_FLOAT, RMS_K_STRING, RMS_K_PAIRSET, RMS_K_POS, RMS_K_IDENT };

struct RmsInst {
	uint8_t	op, kind;
	uint16_t	len;		// RMS_K_STRING: bytes; SCL of mismatches( string, pattern ): its expression
	int32_t	a;		// int; index of the double, pair set or variable; offset in the pool; jump target; builtin; MAT: its expression
};

struct RmsVar {
	int32_t	type;		// RMS_T_*
	int32_t	lo, hi;		// int: lo; float: the double's words; string: offset in the pool, length
};

struct RmsElem {
	int32_t	type;		// Strel::type (SYM_*)
	int32_t	index;		// Strel::index
	int32_t	tag_off, tag_len;	// in the pool; tag_len < 0: no tag
	int32_t	n_mates, mates[ 3 ];	// rows of this table
	int32_t	ps;		// its pair set, or -1
};

struct RmsImage {
	uint32_t	magic;
	int32_t	bytes;
	int32_t	n_inst, n_dbl, n_vars, n_xd, n_elems, n_rows, n_ps, n_efn, n_pool;
	int32_t	stack;		// slots of the operand stack
	int32_t	x_off;		// 1: the explicit left context is rm_xdescr[ 0 ]
	int32_t	ctx_off, efn_off, stride;	// of the hit record
	int32_t	sym_se, sym_ss;	// SYM_SE, SYM_SS
	int32_t	v_score, v_comp, v_pos, v_len, v_slen;	// variables of these names, or -1
	int32_t	o_inst, o_dbl, o_vars, o_xd, o_rows, o_ps, o_efn, o_pool;
	int32_t	flags;		// RMS_IMG_*
	int32_t	bits_L;		// bits() reads at most this many bases: its table (ScoreImage::bits_tab) ends there
	int32_t	n_expr;		// RMS_IMG_MATCH: expressions of the table behind the pool (0: no table); the word the header's alignment left free
};
static_assert( sizeof( RmsImage ) == 136, "the header ends where the first part begins" );
// the image may hold sprintf() and bits(); string + concatenates; a lane has a heap (rm_score_core.h)
#define RMS_IMG_TEXT	1
enum { RMS_BITS_MAX_L = 1024, RMS_DEFAULT_HEAP = 256 };
// the image may hold =~ / !~ (MAT) and mismatches( string, pattern ), each with an expression compiled when it was made
#define RMS_IMG_MATCH	2

struct RmsMatchExpr {
	int32_t	anchored;	// *pat == '^'
	int32_t	first, n_ops;	// its ops among the table's; n_ops < 0: "", which compile() has no expression for -- nothing matches, no mismatch is counted
	int32_t	pat_len;	// strlen( pat ): mismatches() allows 20 * pat_len
};
struct RmsMatch {
	int32_t	n_ops;		// of all expressions
	int32_t	frames;		// frames of the matcher's stack: the most repeating ops of one expression
	// RmsMatchExpr expr[ n_expr ], RmqOp ops[ n_ops ] behind it
};
static_assert( sizeof( RmsMatchExpr ) == 16 && sizeof( RmsMatch ) == 8, "the table is packed" );
RMQ_FN const RmsMatch *rms_match( const RmsImage *m )
{
	return reinterpret_cast<const RmsMatch *>( reinterpret_cast<const char *>( m ) + ( ( m->o_pool + m->n_pool + 7 ) & ~7 ) );
}
RMQ_FN const RmsMatchExpr *rms_match_expr( const RmsImage *m ) { return reinterpret_cast<const RmsMatchExpr *>( rms_match( m ) + 1 ); }
RMQ_FN const RmqOp *rms_match_ops( const RmsImage *m ) { return reinterpret_cast<const RmqOp *>( rms_match_expr( m ) + m->n_expr ); }
// frames of an image's matcher, -1 where it has none: such an image takes no match planes and runs the kernels without
RMQ_FN int rms_frames( const RmsImage *m ) { return ( m->flags & RMS_IMG_MATCH ) && m->n_expr > 0 ? rms_match( m )->frames : -1; }

// bytes of LDS a wave's planes take: three words a stack slot and variable, a byte a slot of the element stack
constexpr int rms_wave_bytes( int stack, int n_vars ) { return ( stack + n_vars ) * 3 * 64 * 4 + RMS_ESTK * 64; }
// the same with the matcher's planes behind them (rmq_wave_bytes, rm_seqcheck.h); frames < 0: no matcher
constexpr int rms_wave_bytes( int stack, int n_vars, int frames ) { return rms_wave_bytes( stack, n_vars ) + ( frames < 0 ? 0 : rmq_wave_bytes( frames ) ); }

#ifndef RMS_POD_ONLY
// ---- the host's half (rm_score_image.cpp)
#include <memory>
#include <string>
#include <vector>

struct RmsResult;
namespace rma {

struct Descriptor;

struct ScoreImage {
	std::vector<uint64_t>	blob;			// the image, 8-byte aligned
	const RmsImage	*image() const { return reinterpret_cast<const RmsImage *>( blob.data() ); }
	std::vector<std::string>	files;		// of the instructions
	std::vector<int32_t>	file_of, line_of;	// per instruction
	std::vector<std::string>	var_names;
	std::string	wdfname;			// the descriptor file strid()'s words name
	std::unique_ptr<rma_program_t>	prog;		// the descriptor's program: a scanner's must be the same, byte for byte
	uint64_t	serial = 0;			// of this image among all that were made (a scanner keeps the last one's on its device)
	int	deepest = 0;				// the deepest operand stack MAIN can reach
	// RMS_IMG_TEXT: 3.32192809488736234789 * log10( 1.0 * b / len ) at ( len - 1 ) * len / 2 + b - 1 for 1 <= b <= len <= bits_L,
	// by this host's log10 in the host VM's expression (do_bits); a scanner uploads it behind the image
	std::vector<double>	bits_tab;
};

// The image of d's MAIN program, made from a private copy of d compiled as ParallelReplayer compiles its workers'
// (BEGIN run on the copy; d itself untouched).  Returns "" or, with no image made, why not.  checked: a loose descriptor
// is not refused -- the caller's records have passed rma_seqcheck_hits (rm_seqcheck.h) and are its fixed rows.
std::string	score_image_make( const Descriptor &d, const rma_program_t &prog, ScoreImage *out, bool checked = false );
// the same by flags (RMA_SCORE_CHECKED 1: as checked; RMA_SCORE_TEXT 2: sprintf() and bits() are not refused, the image has
// RMS_IMG_TEXT and its table; a constant format with %e %E %g %G is refused; RMA_SCORE_MATCH 8: =~, !~ and mismatches( string,
// pattern ) are not refused where the pattern is one string constant compile() takes, the image has RMS_IMG_MATCH)
std::string	score_image_make_flags( const Descriptor &d, const rma_program_t &prog, ScoreImage *out, unsigned flags );
// the host VM's words for a stop
std::string	score_stop_text( const ScoreImage &img, const RmsResult &r );

}	// namespace rma

struct rma_score {
	rma::ScoreImage	img;
};
#endif
