// tests/hostsim/bitvec_check.cpp -- TEST INFRASTRUCTURE: the bit vector helpers of rm_scan_core.h that the search
// kernel's pre-filters use, compiled for the host.  rmd_or_window() against the loop over rmd_peek() it replaces,
// on vectors held in heap blocks of exactly their size (so that a build with -fsanitize=address sees a read
// past either end).  Prints "or_window <cases> mismatches <n>"; exit status 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rm_scan_core.h"

static uint64_t	rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return rng_state;
}

static unsigned long long or_loop( const unsigned long long *v, int x, int lo, int hi, int vec_bits )
{
	unsigned long long	r = 0;
	for( int d = lo; d <= hi; d++ )
		r |= ( x + d >= 0 && x + d + 96 <= vec_bits ) ? rmd_bits64( v, x + d ) : ~0ull;
	return r;
}

static long long check_or_window( long long *bad )
{
	static const int	sizes[] = { 128, 192, 8256 }, widths[] = { -1, 0, 1, 17, 31, 32, 63, 64, 65, 127, 300 }, los[] = { -40, -3, 0, 4, 77 };
	static const double	dens[] = { 0.0, 0.02, 0.5, 1.0 };
	long long	n = 0;
	for( int vec_bits : sizes )
		for( double p : dens ){
			std::vector<unsigned long long>	v( vec_bits / 64 );
			for( auto &w : v ){
				w = 0;
				for( int b = 0; b < 64; b++ )
					if( p >= 1.0 || double( rnd() >> 11 ) / 9007199254740992.0 < p )
						w |= 1ull << b;
			}
			for( int x = -70; x <= vec_bits + 70; x++ )
				for( int lo : los )
					for( int wd : widths ){
						const unsigned long long	got = rmd_or_window( v.data(), x, lo, lo + wd, vec_bits );
						const unsigned long long	want = or_loop( v.data(), x, lo, lo + wd, vec_bits );
						n++;
						if( got != want && ( *bad )++ < 10 )
							fprintf( stderr, "or_window: vec_bits %d density %g x %d lo %d hi %d: %016llx, the loop %016llx\n",
								vec_bits, p, x, lo, lo + wd, got, want );
					}
		}
	return n;
}

int main()
{
	long long	bad = 0;
	const long long	n = check_or_window( &bad );
	printf( "or_window %lld mismatches %lld\n", n, bad );
	return bad ? 1 : 0;
}
