// start_compact_check.cpp -- TEST INFRASTRUCTURE.
//
// The pre-filter of the search kernel that walks nothing (rm_scan_kernel.h, RMK_LEAN_FLUSH / RMK_LEAN_CONCAT_FLUSH) takes the
// start positions out of the start vector by one prefix sum a wave: every lane counts the bits of its 16 positions, gets its
// place among the wave's, and stores its own positions into the wave's buffer of 128 places, from which 64 are taken whenever
// 64 wait; what the buffer cannot hold yet stays in the lane.  The other lean instances hand the bits on in rounds of
// ballots, one bit a lane.  Here both, statement for statement, a wave as 64 lanes one after the other, the buffer in a heap
// block of exactly its size (a build with -fsanitize=address sees a store past either end):
//
//   start_compact_check [SEED]
//     random words of every density, 0 .. 16 bits a lane, some lanes full beside empty ones, one to four steps a tile; the
//     prefix sum must hand on the same set of start positions per wave as the rounds of ballots, each exactly once, 64 at a
//     time but for the last hand-off, in as many hand-offs.
//     Prints "compact waves N positions P rounds R differ D"; exit status 1 when anything differs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

// A wave of the pre-filter's start_vec block: 64 lanes, 16 bits of the start vector each, a buffer of 128 places from which
// 64 positions are taken whenever 64 wait.  `taken` receives what take() hands to body(), round by round.
struct Wave {
	std::unique_ptr<uint16_t[]>	cbuf{ new uint16_t[ 128 ] };
	int	n_wait = 0;
	std::vector<std::vector<int>>	taken;
	void take()
	{
		const int	n_take = n_wait < 64 ? n_wait : 64, rest = n_wait - n_take;
		taken.emplace_back( cbuf.get(), cbuf.get() + n_take );
		std::vector<uint16_t>	moved( cbuf.get() + n_take, cbuf.get() + n_take + rest );
		std::copy( moved.begin(), moved.end(), cbuf.get() );
		n_wait = rest;
	}
};

// the rounds of ballots (the instances that walk; the flush instances until now)
static void step_ballot( Wave &wv, const unsigned *m_in, int rel_lo0 )
{
	unsigned	m[ 64 ];
	std::copy( m_in, m_in + 64, m );
	for( ;; ){
		bool	any = false;
		for( int l = 0; l < 64; l++ )
			any = any || m[ l ] != 0;
		if( !any )
			break;
		int	n = 0;
		for( int l = 0; l < 64; l++ )
			if( m[ l ] ){
				wv.cbuf[ wv.n_wait + n++ ] = uint16_t( rel_lo0 + 16 * l + __builtin_ctz( m[ l ] ) );
				m[ l ] &= m[ l ] - 1;
			}
		wv.n_wait += n;
		while( wv.n_wait >= 64 )
			wv.take();
	}
}

// one prefix sum over the lanes' counts, every lane stores its own positions: rm_scan_kernel.h, `if constexpr( !WALK )` of
// the start_vec block, statement for statement (the lanes of a chunk one after the other: they write different places)
static void step_prefix( Wave &wv, const unsigned *m_in, int rel_lo0 )
{
	unsigned	m[ 64 ];
	int	at[ 64 ], tot = 0;
	for( int l = 0; l < 64; l++ ){
		m[ l ] = m_in[ l ];
		at[ l ] = tot;
		tot += __builtin_popcount( m[ l ] );
	}
	for( int base = 0; base < tot; ){
		const int	lim = base + ( 128 - wv.n_wait );
		for( int l = 0; l < 64; l++ )
			while( m[ l ] && at[ l ] < lim ){
				wv.cbuf[ wv.n_wait + at[ l ] - base ] = uint16_t( rel_lo0 + 16 * l + __builtin_ctz( m[ l ] ) );
				m[ l ] &= m[ l ] - 1;
				at[ l ]++;
			}
		const int	add = std::min( tot, lim ) - base;
		wv.n_wait += add;
		base += add;
		while( wv.n_wait >= 64 )
			wv.take();
	}
}

static int compact( unsigned seed )
{
	std::mt19937_64	rng( seed );
	long long	n_waves = 0, n_pos = 0, n_differ = 0, n_rounds = 0;
	for( int dens = 0; dens <= 16; dens++ )		// bits a lane on average, 0 .. 16 of 16
		for( int rep = 0; rep < 200; rep++ ){
			Wave	a, b;
			std::vector<int>	all;
			// a tile's steps: 1024 positions of the wave a step
			const int	n_steps = 1 + int( rng() % 4 );
			for( int s = 0; s < n_steps; s++ ){
				unsigned	m[ 64 ];
				for( int l = 0; l < 64; l++ ){
					m[ l ] = 0;
					for( int i = 0; i < 16; i++ )
						if( int( rng() % 16 ) < dens || ( rep % 7 == 0 && l % 5 == 0 && dens > 0 ) )		// (some lanes full beside empty ones)
							m[ l ] |= 1u << i;
					for( int i = 0; i < 16; i++ )
						if( ( m[ l ] >> i ) & 1u )
							all.push_back( 1024 * s + 16 * l + i );
				}
				step_ballot( a, m, 1024 * s );
				step_prefix( b, m, 1024 * s );
			}
			while( a.n_wait > 0 )
				a.take();
			while( b.n_wait > 0 )
				b.take();
			n_waves++;
			n_pos += ( long long )all.size();
			n_rounds += ( long long )b.taken.size();
			// every position exactly once, both ways; the hand-offs 64 at a time but for the last
			std::vector<int>	sa, sb;
			for( const auto &r : a.taken )
				sa.insert( sa.end(), r.begin(), r.end() );
			for( size_t i = 0; i < b.taken.size(); i++ ){
				sb.insert( sb.end(), b.taken[ i ].begin(), b.taken[ i ].end() );
				if( i + 1 < b.taken.size() && b.taken[ i ].size() != 64 )
					n_differ++;
			}
			std::sort( sa.begin(), sa.end() );
			std::sort( sb.begin(), sb.end() );
			if( ( sa != all || sb != all || a.taken.size() != b.taken.size() ) && n_differ++ < 10 )
				fprintf( stderr, "compact: density %d rep %d: %zu positions, %zu by ballots in %zu rounds, %zu by prefix sum in %zu rounds\n", dens, rep,
					all.size(), sa.size(), a.taken.size(), sb.size(), b.taken.size() );
		}
	printf( "compact waves %lld positions %lld rounds %lld differ %lld\n", n_waves, n_pos, n_rounds, n_differ );
	return n_differ ? 1 : 0;
}

int main( int argc, char **argv )
{
	return compact( argc > 1 ? unsigned( atoi( argv[ 1 ] ) ) : 1u );
}
