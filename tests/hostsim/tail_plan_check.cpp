// tests/hostsim/tail_plan_check.cpp -- TEST INFRASTRUCTURE, not product code.
//
// plan_tail() and tail_verdict() of rnamotif_amd/csrc/rm_tail_plan.h over their edges: the rule by which a scan's tail is
// enqueued ahead of the count, and the rule by which the scan's end takes its records or does the tail again.  A stand-alone
// program without a HIP call; tests/test_tail_plan_cpu.py builds and runs it, once more with -fsanitize=address,undefined.
// Exit status 0 and "tail_plan_check: ok" when every check holds; a line per check that does not.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "rm_tail_plan.h"

static int	g_failed = 0;
#define CHECK( cond )	do{ if( !( cond ) ){ printf( "line %d: %s\n", __LINE__, #cond ); g_failed++; } }while( 0 )

using namespace rma;

int main()
{
	const int64_t	CAP = int64_t( 1 ) << 17;
	const TailOpts	rule;		// every option as a scanner has it when nothing was set

	// ---- plan_tail
	// no earlier scan: nothing is planned
	CHECK( !plan_tail( -1, CAP, rule ).speculate );
	CHECK( plan_tail( -1, CAP, rule ).n_sort == 0 );
	// an earlier scan without records, with one, with few: the least a tail is planned for
	for( int64_t cm : { int64_t( 0 ), int64_t( 1 ), int64_t( 2 ), int64_t( 819 ) } ){
		const TailPlan	p = plan_tail( cm, CAP, rule );
		CHECK( p.speculate && p.n_sort == RMA_TAIL_MIN );
	}
	// a quarter above the most records seen, where that is more than the least
	CHECK( plan_tail( 820, CAP, rule ).n_sort == 1025 );
	CHECK( plan_tail( 5837, CAP, rule ).n_sort == 5837 + 1459 );
	CHECK( plan_tail( 100000, CAP, rule ).n_sort == 125000 );
	// the hit buffer below the margin: all of it, no more
	CHECK( plan_tail( 104858, CAP, rule ).n_sort == CAP );		// 104858 + 26214 = 131072
	CHECK( plan_tail( 104857, CAP, rule ).n_sort == CAP - 1 );		// 104857 + 26214
	CHECK( plan_tail( CAP - 1, CAP, rule ).n_sort == CAP );
	CHECK( plan_tail( 3 * CAP, CAP, rule ).n_sort == CAP );
	CHECK( plan_tail( 10, 600, rule ).speculate && plan_tail( 10, 600, rule ).n_sort == 600 );	// (below the least, too)
	CHECK( !plan_tail( 10, 1, rule ).speculate && !plan_tail( 10, 0, rule ).speculate );
	// the same plan for every count up to what is remembered
	CHECK( plan_tail( 5837, CAP, rule ).n_sort == plan_tail( std::max<int64_t>( 5837, 5700 ), CAP, rule ).n_sort );
	// the switches: each of them alone turns it off, whatever was seen
	{
		TailOpts	o;
		o.spec_tail = 0;
		CHECK( !plan_tail( 5837, CAP, o ).speculate && plan_tail( 5837, CAP, o ).n_sort == 0 );
		o = TailOpts();
		o.dbg = 2;
		CHECK( !plan_tail( 5837, CAP, o ).speculate );
		o = TailOpts();
		o.timing = 1;
		CHECK( !plan_tail( 5837, CAP, o ).speculate );
		o = TailOpts();
		o.host_sort = 1;
		CHECK( !plan_tail( 5837, CAP, o ).speculate );
		o = TailOpts();
		o.timed_apart = true;
		CHECK( !plan_tail( 5837, CAP, o ).speculate );
	}

	// ---- tail_seen: the last count, or half of what was remembered
	CHECK( tail_seen( -1, 0 ) == 0 && tail_seen( -1, 77 ) == 77 );
	CHECK( tail_seen( 5837, 5837 ) == 5837 && tail_seen( 5837, 5900 ) == 5900 && tail_seen( 5837, 5000 ) == 5000 );
	CHECK( tail_seen( 5837, 2918 ) == 2918 && tail_seen( 5837, 2917 ) == 2918 && tail_seen( 1000000, 0 ) == 500000 );
	CHECK( tail_seen( 1, 0 ) == 0 && tail_seen( 0, 0 ) == 0 );
	{
		int64_t	seen = 1000000;		// one scan with many records, then none: the plan is back at its least after ten scans
		int	scans = 0;
		while( plan_tail( seen, CAP * 16, rule ).n_sort > RMA_TAIL_MIN && scans < 100 ){
			seen = tail_seen( seen, 0 );
			scans++;
		}
		CHECK( scans == 11 );
	}

	// ---- tail_verdict
	const TailRepeat	none;
	const int64_t	N = 7296;
	CHECK( tail_verdict( 5837, N, CAP, none, false, 5837 ) == TAIL_TAKE );
	// the plan's edge
	CHECK( tail_verdict( N - 1, N, CAP, none, false, N - 1 ) == TAIL_TAKE );
	CHECK( tail_verdict( N, N, CAP, none, false, N ) == TAIL_TAKE );
	CHECK( tail_verdict( N + 1, N, CAP, none, false, N + 1 ) == TAIL_REDO );
	// the hit buffer's edge, planned for all of it
	CHECK( tail_verdict( CAP, CAP, CAP, none, false, CAP ) == TAIL_TAKE );
	CHECK( tail_verdict( CAP + 1, CAP, CAP, none, false, CAP + 1 ) == TAIL_REDO );
	CHECK( tail_verdict( CAP + 1, CAP + 5, CAP, none, false, CAP + 1 ) == TAIL_REDO );	// (a plan beyond the buffer does not help)
	CHECK( tail_verdict( ~0ull, N, CAP, none, false, 5 ) == TAIL_REDO );
	// every repeat condition, alone and together
	for( int m = 1; m < 16; m++ ){
		TailRepeat	r;
		r.queue_need = m & 1;
		r.flush_queue_need = m & 2;
		r.list_need = m & 4;
		r.piece_overflow = m & 8;
		CHECK( r.any() );
		CHECK( tail_verdict( 5837, N, CAP, r, false, 5837 ) == TAIL_REDO );
	}
	CHECK( !none.any() );
	// the ordering's flag
	CHECK( tail_verdict( 5837, N, CAP, none, true, 5837 ) == TAIL_REDO );
	// no records, one record: their own ways out; two are the fewest taken
	CHECK( tail_verdict( 0, N, CAP, none, false, 0 ) == TAIL_REDO );
	CHECK( tail_verdict( 1, N, CAP, none, false, 1 ) == TAIL_REDO );
	CHECK( tail_verdict( 2, N, CAP, none, false, 2 ) == TAIL_TAKE );
	// records that are not the count (a caller that says so is not given the tail's)
	CHECK( tail_verdict( 5837, N, CAP, none, false, 5836 ) == TAIL_REDO );
	CHECK( tail_verdict( 5837, -1, CAP, none, false, 5837 ) == TAIL_REDO && tail_verdict( 5837, N, -1, none, false, 5837 ) == TAIL_REDO );

	// ---- the two together, as a scanner uses them: counts in heap blocks of exactly their number
	{
		const std::vector<int64_t>	counts{ 0, 3, 900, 1024, 1025, 1300, 1281, 1282, 5837, 5837, 7296, 7297, 2, 1, 0, CAP, CAP + 1, CAP };
		std::vector<int>	taken( counts.size() );
		int64_t	count_max = -1;
		for( size_t i = 0; i < counts.size(); i++ ){
			const TailPlan	p = plan_tail( count_max, CAP, rule );
			taken[ i ] = p.speculate && tail_verdict( ( unsigned long long )counts[ i ], p.n_sort, CAP, none, false, counts[ i ] ) == TAIL_TAKE;
			count_max = tail_seen( count_max, counts[ i ] );
		}
		// plans: none, 1024, 1024, 1125, 1280, 1281, 1625, 1601, 1602, 7296, 7296, 9120, 9121, 4560, 2280, 1140, CAP, CAP
		//                         0  3  900 1024 1025 1300 1281 1282 5837 5837 7296 7297 2  1  0  CAP CAP+1 CAP
		const std::vector<int>	want{ 0, 1, 1,  1,   1,   0,   1,   1,   0,   1,   1,   1,   1, 0, 0, 0,  0,    1 };
		CHECK( want.size() == counts.size() );
		for( size_t i = 0; i < counts.size(); i++ )
			if( taken[ i ] != want[ i ] ){
				printf( "scan %zu of %lld records: taken %d, expected %d\n", i, ( long long )counts[ i ], taken[ i ], want[ i ] );
				g_failed++;
			}
	}
	if( g_failed == 0 )
		printf( "tail_plan_check: ok\n" );
	return g_failed != 0;
}
