// rm_structenergy.h -- efn() and efn2() of structures given base by base (rma_structure_energies, rm_hitpost.cpp): the
// rule that accepts a structure, the candidate view the cores rm_efn_core.h / rm_efn2_core.h walk, and the two calls.
// Compiled for the device by rm_structenergy_dev.hip and for the host by rm_hitpost.cpp (the words of a refusal) and
// tests/hostsim/struct_energy_check.cpp.
//
// A structure is `len` letters and `len` partners: pair( i ) is the index inside the structure of the base that i
// pairs with, or -1 (the convention of rma_hit_structures' mate).  Pairs are taken as given, as the reference's efn_drv
// and efn2_drv take a .ct file: no pair set filters them, a . a counts as a pair.
//
// Refused, with the structure's index: offsets that are not an ascending cut of [0, total), more than RMSE_MAX_BASES
// bases (so that no loop size is ever clamped to the logarithm tables' RMA_EFN_LOGINC entries), a partner outside the
// structure, a base paired with itself, a pair that its partner does not return, more than RMSE_MAX_HELICES helices
// (the cores' large stacks are sized for the fifty a descriptor can have).  A helix is counted as a descriptor would
// need one: a pair (i, j) opens a new helix unless (i-1, j+1) is a pair.
//
// Accepted and answered with both infinities without a walk of the cores (rmse_base_t::inf):
//   crossing pairs   The cores return infinity from several places when a walk meets a partner outside its interval,
//                    but add it to what the callers of the interval hold (rm_efn_core.h "knot"): the sum is not the
//                    constant, and efn2's walk of a closed loop trusts that the next helix is there.
//   a pair (i, i+1)  It closes no loop.  The reference's walk of the helix runs on past it with i > j and indexes its
//                    hairpin table with a negative size: where the reference leaves its arrays the answer is
//                    infinity, as for efn2's exterior loop (rm_efn2_core.h).
#pragma once
#include "rm_efn_core.h"
#include "rm_efn2_core.h"

#define RMSE_CACHE		96				// bases whose codes and partners a lane keeps in LDS: rm_scan_kernel.h's EFN_CACHE
#define RMSE_MAX_BASES		( RMA_EFN_LOGINC - 1 )
#define RMSE_MAX_HELICES	50
#define RMSE_SMALL_HELICES	15				// more: the instance with the large stacks (BIG), as rmd_program_t::efn_big
#define RMSE_INFO_INF		0x100				// a structure's info word: helices | RMSE_INFO_INF

enum {
	RMSE_OK = 0,
	RMSE_OFF_FIRST,		// off[ 0 ] != 0
	RMSE_OFF_DECREASES,	// off[ s + 1 ] < off[ s ]
	RMSE_OFF_OUTSIDE,	// [ off[ s ], off[ s + 1 ] ) not inside [ 0, total )
	RMSE_OFF_LAST,		// off[ n ] != total
	RMSE_TOO_LONG,		// more than RMSE_MAX_BASES bases
	RMSE_PAIR_RANGE,	// a partner that is neither -1 nor inside the structure
	RMSE_PAIR_SELF,		// a base paired with itself
	RMSE_PAIR_ASYM,		// pair( pair( i ) ) != i
	RMSE_HELICES		// more than RMSE_MAX_HELICES helices
};

// structure s of n: its bases are [ lo, hi ) = [ off[ s ], off[ s + 1 ] ) of `total`
RMD_FN int rmse_check_offsets( long long lo, long long hi, long long s, long long n, long long total )
{
	if( s == 0 && lo != 0 )
		return RMSE_OFF_FIRST;
	if( hi < lo )
		return RMSE_OFF_DECREASES;
	if( lo < 0 || hi > total )
		return RMSE_OFF_OUTSIDE;
	if( s == n - 1 && hi != total )
		return RMSE_OFF_LAST;
	if( hi - lo > RMSE_MAX_BASES )
		return RMSE_TOO_LONG;
	return RMSE_OK;
}

// the partners of one structure where the caller has them: every `stride` words
struct rmse_pairs_t {
	const int32_t	*p;
	long long	stride;
	RMD_FN_MEMBER int	operator()( int i ) const { return p[ i * stride ]; }
};

// What base i says of its structure.  bad: a reason to refuse it; helix: i opens a helix; inf: i opens a pair that makes
// the energies infinite (see above).  The walk behind `inf` steps through the loop the pair (i, j) closes -- unpaired
// bases one by one, inner pairs in one step -- and must arrive at j exactly; it reads partners as they are, checked or
// not, and ends whatever they hold: every step moves forward and none goes past j.  Over a nested structure the walks
// of all pairs together take each base once.
struct rmse_base_t {
	int	bad, helix, inf;
};
template< class Pairs > RMD_FN rmse_base_t rmse_check_base( const Pairs &pair, int len, int i )
{
	rmse_base_t	r = { RMSE_OK, 0, 0 };
	const int	j = pair( i );
	if( j == -1 )
		return r;
	if( j < 0 || j >= len )
		r.bad = RMSE_PAIR_RANGE;
	else if( j == i )
		r.bad = RMSE_PAIR_SELF;
	else if( pair( j ) != i )
		r.bad = RMSE_PAIR_ASYM;
	if( r.bad != RMSE_OK || j < i )
		return r;
	r.helix = !( i > 0 && pair( i - 1 ) == j + 1 );
	if( j == i + 1 )
		r.inf = 1;
	for( int k = i + 1; k < j; ){
		const int	q = pair( k );
		if( q == -1 )
			k++;
		else if( q > k && q < j )
			k = q + 1;
		else{
			r.inf = 1;
			break;
		}
	}
	return r;
}

// A whole structure, base by base (the device gives a wave's lanes a base each, rm_structenergy_dev.hip): the reason to
// refuse it with *which = the first base that has one (RMSE_HELICES: the number of helices), or RMSE_OK with
// *info = helices | RMSE_INFO_INF.
template< class Pairs > RMD_FN int rmse_check_structure( const Pairs &pair, int len, int *which, int *info )
{
	int	helices = 0, inf = 0;
	for( int i = 0; i < len; i++ ){
		const rmse_base_t	b = rmse_check_base( pair, len, i );
		if( b.bad != RMSE_OK ){
			*which = i;
			return b.bad;
		}
		helices += b.helix;
		inf |= b.inf;
	}
	*which = helices;
	if( helices > RMSE_MAX_HELICES )
		return RMSE_HELICES;
	*info = helices | ( inf ? RMSE_INFO_INF : 0 );
	return RMSE_OK;
}
// which instance of the cores a checked structure takes
RMD_FN int rmse_info_big( int info ) { return !( info & RMSE_INFO_INF ) && ( info & 0xff ) > RMSE_SMALL_HELICES; }

// byte -> base code through the letter the byte stands for: a c g t/u in either case 0..3, anything else RMA_BC_N
RMD_FN int rmse_letter_code( unsigned char letter )
{
	switch( letter ){
	case 'a' : case 'A' : return RMA_BC_A;
	case 'c' : case 'C' : return RMA_BC_C;
	case 'g' : case 'G' : return RMA_BC_G;
	case 't' : case 'T' : case 'u' : case 'U' : return RMA_BC_T;
	default : return RMA_BC_N;
	}
}

// The candidate view of the cores (rm_efn_core.h: len, bc( i ), bp( i )) over a checked structure: its letters and
// partners where the caller has them, the 256 codes of its bytes, and -- optional, as rme_cand_t's -- the codes and
// partners of the whole structure in arrays of the caller's (the kernel: in LDS, for structures of up to RMSE_CACHE bases).
struct rme_struct_cand_t {
	const uint8_t	*base;
	rmse_pairs_t	pair;
	const uint8_t	*code;		// [ 256 ]
	int	len;
	int16_t	*cbp = nullptr;
	uint8_t	*cbc = nullptr;

	RMD_FN_MEMBER void	fill_cache( int16_t *bpbuf, uint8_t *bcbuf )
	{
		for( int i = 0; i < len; i++ ){
			bcbuf[ i ] = code[ base[ i ] ];
			bpbuf[ i ] = int16_t( pair( i ) );
		}
		cbp = bpbuf;
		cbc = bcbuf;
	}
	RMD_FN_MEMBER int	bc( int i ) const
	{
		if( i < 0 || i >= len )
			return RMA_BC_N;
		return cbc != nullptr ? cbc[ i ] : code[ base[ i ] ];
	}
	RMD_FN_MEMBER int	bp( int i ) const
	{
		if( i < 0 || i >= len )
			return -1;
		return cbp != nullptr ? cbp[ i ] : pair( i );
	}
};

// efn() / efn2() of the whole structure: RM_efn( 0, len - 1, 1 ) / RM_efn2() as the drivers call them.  BIG as rme_ctx_t's.
template< int BIG > RMD_FN int rme_struct_energy( const rme_tables_t *T, const rme_struct_cand_t &c )
{
	if( c.len <= 0 )
		return RME_INF;
	rme_ctx_t< rme_struct_cand_t, BIG >	x;
	x.T = T;
	x.C = &c;
	x.l_base = c.len - 1;
	return rme_efn( x );
}
template< int BIG > RMD_FN int rme2_struct_energy( const rma_efn2data_t *E, const rme_struct_cand_t &c )
{
	if( c.len <= 0 )
		return RME2_INF;
	rme2_ctx_t< rme_struct_cand_t, BIG >	x;
	x.E = E;
	x.C = &c;
	x.l_base = c.len - 1;
	return rme2_efn2( x );
}
