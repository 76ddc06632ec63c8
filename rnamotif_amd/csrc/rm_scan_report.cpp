// rm_scan_report.cpp -- the [dbg] lines of a scan, from a host copy of the counter block.  Which name a slot
// goes by depends on the kernel that wrote it (rm_diag.h): the general instances, the lean ones, the drain kernel.
#include <cstdio>
#include "rm_scan_report.h"

namespace rma {

void debug_report( const unsigned long long *c, const ScanShape &s, const rmd_program_t &dp )
{
	const int	dbg = s.dbg;
	fprintf( stderr, "[dbg] queued items: %llu, candidates %llu (tile %d x %d, queue %d, LDS %zu, %lld tiles)\n", c[ RMK_C_QUEUED ], c[ RMK_C_COUNT ],
		s.tile_t, s.group, s.qcap, s.lds, s.n_tiles );
	if( ( dbg & RMK_DBG_TIMELINE ) && s.lean ){
		const double	t0 = double( ~c[ RMK_C_TL_START ] ), g = double( c[ RMK_C_TL_WGS ] );
		fprintf( stderr, "[dbg] workgroups that had tiles (%.0f of %d): out of tiles after %.1f us (mean), done after %.1f us (mean), %.1f us (last)\n", g, s.grid,
			( double( c[ RMK_C_TL_DRY_SUM ] ) / g - t0 ) * 0.01, ( double( c[ RMK_C_TL_DONE_SUM ] ) / g - t0 ) * 0.01, ( double( c[ RMK_C_TL_DONE_MAX ] ) - t0 ) * 0.01 );
	}
	if( ( dbg & RMK_DBG_DRAIN_DONE ) && s.drained ){
		const unsigned long long	*bins = c + RMK_C_DRAIN_DONE;
		fprintf( stderr, "[dbg] drain: waves through by 16 us from the first wave's start:" );
		for( int b = 0; b < RMK_CN_LOG2_BINS; b++ )
			if( bins[ b ] )
				fprintf( stderr, " %d:%llu", b, bins[ b ] );
		fprintf( stderr, "\n" );
	}
	if( dbg & RMK_DBG_CYCLES ){
		const unsigned long long	*ph = c + RMK_C_PHASE;
		double	tot = 0;
		for( int i = 0; i < RMK_CN_PHASES; i++ )
			tot += double( ph[ i ] );
		const bool	lean = s.lean, drained = s.drained;
		if( lean && !drained )
			fprintf( stderr, "[dbg] pool sessions: %.3g wave cycles popping (%.0f per round), %.3g stepping (%.0f per step)\n",
				double( c[ RMK_C_POP_CYCLES ] ), c[ RMK_C_POP_ROUNDS ] ? double( c[ RMK_C_POP_CYCLES ] ) / c[ RMK_C_POP_ROUNDS ] : 0.0,
				double( c[ RMK_C_STEP_CYCLES ] ), c[ RMK_C_STEPS ] ? double( c[ RMK_C_STEP_CYCLES ] ) / c[ RMK_C_STEPS ] : 0.0 ),
			fprintf( stderr, "[dbg] longest step %.3g cycles, most stepping in one wave (one session) %.3g cycles\n", double( c[ RMK_C_STEP_LONGEST ] ), double( c[ RMK_C_WAVE_MOST ] ) );
		if( drained ){
			// (the drain kernel's items)
			const unsigned long long	items = c[ RMK_C_DRAIN_ITEMS ];
			fprintf( stderr, "[dbg] drain: %llu items in the list (%llu taken), %llu walked: %.0f cycles and %.1f steps each; longest %.3g cycles, most steps %llu\n",
				c[ RMK_C_LIST_RESERVED ], c[ RMK_C_LIST_TAKEN ], items, items ? double( c[ RMK_C_DRAIN_CYCLES ] ) / items : 0.0,
				items ? double( c[ RMK_C_DRAIN_STEPS ] ) / items : 0.0, double( c[ RMK_C_DRAIN_LONGEST ] ), c[ RMK_C_DRAIN_MOST_STEPS ] );
			{
				// (taking items, stepping, complete matches, hand-overs)
				const unsigned long long	*lap = c + RMK_C_DRAIN_LAP, rounds = c[ RMK_C_DRAIN_ROUNDS ];
				const double	all = double( lap[ 0 ] + lap[ 1 ] + lap[ 2 ] + lap[ 3 ] ) + 1;
				fprintf( stderr, "[dbg] drain: %llu wave rounds of %.1f lanes; wave cycles taking items %.1f%%, stepping %.1f%%, complete matches %.1f%%, hand-overs %.1f%%; %.0f cycles a round\n",
					rounds, rounds ? double( c[ RMK_C_DRAIN_LANES ] ) / rounds : 0.0, 100 * lap[ 0 ] / all, 100 * lap[ 1 ] / all, 100 * lap[ 2 ] / all, 100 * lap[ 3 ] / all,
					rounds ? all / rounds : 0.0 );
			}
			fprintf( stderr, "[dbg] drain: items by log2( cycles ):" );
			for( int b = 8; b < RMK_CN_LOG2_BINS; b++ )
				if( c[ RMK_C_DRAIN_LOG2 + b ] )
					fprintf( stderr, " %d:%llu", b, c[ RMK_C_DRAIN_LOG2 + b ] );
			fprintf( stderr, "\n[dbg] drain: items by complete matches (0, 1, 2-3, 4-7, ...: count, mean cycles):" );
			for( int kk = 0; kk < RMK_CN_EMIT_BINS; kk++ )
				if( c[ RMK_C_DRAIN_EMIT_ITEMS + kk ] )
					fprintf( stderr, " %llu,%.0f", c[ RMK_C_DRAIN_EMIT_ITEMS + kk ], double( c[ RMK_C_DRAIN_EMIT_CYCLES + kk ] ) / c[ RMK_C_DRAIN_EMIT_ITEMS + kk ] );
			fprintf( stderr, "\n" );
		}else if( lean ){
			fprintf( stderr, "[dbg] steps by log2( cycles ):" );
			for( int b = 8; b < RMK_CN_LOG2_BINS; b++ )
				if( c[ RMK_C_STEP_LOG2 + b ] )
					fprintf( stderr, " %d:%llu", b, c[ RMK_C_STEP_LOG2 + b ] );
			fprintf( stderr, "\n[dbg] complete matches: %llu, %.0f cycles each", c[ RMK_C_EMITTED ], c[ RMK_C_EMITTED ] ? double( c[ RMK_C_EMIT_CYCLES ] ) / c[ RMK_C_EMITTED ] : 0.0 );
			fprintf( stderr, "\n[dbg] steps by deepest level (count, mean cycles):" );
			for( int kk = 0; kk < RMK_CN_LEVEL_BINS; kk++ )
				if( c[ RMK_C_LEVEL_STEPS + kk ] )
					fprintf( stderr, " %d:%llu,%.0f", kk, c[ RMK_C_LEVEL_STEPS + kk ], double( c[ RMK_C_LEVEL_CYCLES + kk ] ) / c[ RMK_C_LEVEL_STEPS + kk ] );
			fprintf( stderr, "\n" );
		}
		if( lean && !drained )
			fprintf( stderr, "[dbg] pass B: %llu pop rounds of %.1f lanes, %llu steps of %.1f lanes; wave cycles popping %.1f%%, stepping %.1f%%\n",
				c[ RMK_C_POP_ROUNDS ], c[ RMK_C_POP_ROUNDS ] ? double( c[ RMK_C_POP_LANES ] ) / c[ RMK_C_POP_ROUNDS ] : 0.0,
				c[ RMK_C_STEPS ], c[ RMK_C_STEPS ] ? double( c[ RMK_C_STEP_LANES ] ) / c[ RMK_C_STEPS ] : 0.0,
				100.0 * c[ RMK_C_POP_CYCLES ] / double( c[ RMK_C_POP_CYCLES ] + c[ RMK_C_STEP_CYCLES ] + 1 ),
				100.0 * c[ RMK_C_STEP_CYCLES ] / double( c[ RMK_C_POP_CYCLES ] + c[ RMK_C_STEP_CYCLES ] + 1 ) );
		for( int kk = 0; kk < dp.n_searches && kk < RMK_CN_GEN_LEVELS && !lean; kk++ ){
			const unsigned long long	*lv = c + RMK_C_GEN_LEVEL + 2 * kk;	// (wave rounds, lanes served)
			fprintf( stderr, "[dbg] level %2d (element %2d, type %d): %llu wave rounds, %.1f lanes each\n", kk, dp.searches[ kk ],
				dp.elems[ dp.searches[ kk ] ].type, lv[ 0 ], lv[ 0 ] ? double( lv[ 1 ] ) / lv[ 0 ] : 0.0 );
		}
		fprintf( stderr, "[dbg] wave cycles: decode %.1f%%, literal %.1f%%, rows %.1f%%, pre-filter %.1f%%, search %.1f%%, waiting %.1f%%\n",
			100 * ph[ 0 ] / tot, 100 * ph[ 1 ] / tot, 100 * ph[ 2 ] / tot, 100 * ph[ 3 ] / tot, 100 * ph[ 4 ] / tot, 100 * ph[ 5 ] / tot );
	}
}

}	// namespace rma
