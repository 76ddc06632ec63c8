// rm_structenergy_dev.hip -- see rm_structenergy_dev.h
#include <algorithm>
#include <hip/hip_runtime.h>
#define RMD_HD		__host__ __device__ inline
#define RMD_FN		static __device__ inline
#define RMD_FN_MEMBER	__device__ inline
#include "rm_structenergy.h"
#include "rm_structenergy_dev.h"

namespace rma {

namespace {

constexpr int	SE_BLOCK = 256;
constexpr int	SE_WAVES = SE_BLOCK / 64;
constexpr int	SE_N16_PAD = ( RME_N16 + 7 ) / 8 * 8;	// (the device copy is padded to a multiple of 8 entries: rma::efn_tables16)
static_assert( RMSE_CACHE < 32768, "a cached partner is an int16" );
static_assert( SE_BLOCK == 256, "a lane stages one of the 256 codes" );

// A wave per structure, grid-stride over the structures.  The loop over s and everything outside the loop over the
// bases runs with the whole wave active: the votes and shuffles see all 64 lanes.  Only partners inside [0, total) of
// `pair` are read: a structure whose offsets would lead outside is refused before its bases are looked at, and
// rmse_check_base reads pair( j ) only for a j inside the structure.
__global__ void __launch_bounds__( SE_BLOCK )
rma_struct_check_kernel( StructBatch b, int32_t *info, unsigned long long *bad )
{
	const int	lane = threadIdx.x & 63;
	for( long long s = blockIdx.x * ( long long )SE_WAVES + ( threadIdx.x >> 6 ); s < b.n; s += gridDim.x * ( long long )SE_WAVES ){
		const long long	lo = b.off[ s ], hi = b.off[ s + 1 ];
		if( rmse_check_offsets( lo, hi, s, b.n, b.total ) != RMSE_OK ){
			if( lane == 0 )
				atomicMin( bad, static_cast<unsigned long long>( s ) );
			continue;
		}
		const int	len = int( hi - lo );
		const rmse_pairs_t	pair{ b.pair + lo * b.pair_stride, b.pair_stride };
		int	refused = 0, helices = 0, inf = 0;
		for( int i = lane; i < len; i += 64 ){
			const rmse_base_t	r = rmse_check_base( pair, len, i );
			refused |= r.bad != RMSE_OK;
			helices += r.helix;
			inf |= r.inf;
		}
		for( int d = 32; d > 0; d >>= 1 )
			helices += __shfl_xor( helices, d );
		refused = __any( refused );
		inf = __any( inf );
		if( lane == 0 ){
			const int	w = helices | ( inf ? RMSE_INFO_INF : 0 );
			if( refused || helices > RMSE_MAX_HELICES )
				atomicMin( bad, static_cast<unsigned long long>( s ) );
			else{
				info[ s ] = w;
				if( rmse_info_big( w ) )
					atomicMax( bad + 1, 1ull );
			}
		}
	}
}

// The staged energy kernel's shape (rm_scan_kernel.h efn_body, STAGE = true) over structures: 60.7 KB of tables,
// 256 bytes of codes and 256 lanes' rows of RMSE_CACHE partners and codes -- 136 KB of LDS, one workgroup a CU.
template< int BIG >
__global__ void __launch_bounds__( SE_BLOCK )
rma_struct_energy_kernel( StructBatch b, const int32_t *info, StructTables g, int32_t *d_efn, int32_t *d_efn2 )
{
	__shared__ __align__( 16 ) int16_t	t16_s[ SE_N16_PAD ];
	__shared__ uint8_t	code_s[ 256 ];
	__shared__ int16_t	s_bp[ SE_BLOCK ][ RMSE_CACHE + 1 ];
	__shared__ uint8_t	s_bc[ SE_BLOCK ][ RMSE_CACHE + 4 ];
	if( g.t16 != nullptr )
		for( int i = threadIdx.x; i < SE_N16_PAD / 8; i += SE_BLOCK )
			reinterpret_cast<uint4 *>( t16_s )[ i ] = reinterpret_cast<const uint4 *>( g.t16 )[ i ];
	code_s[ threadIdx.x ] = g.code[ threadIdx.x ];
	__syncthreads();
	const rme_tables_t	T{ t16_s, g.tlkey, g.loginc };
	const bool	want = d_efn != nullptr && g.t16 != nullptr, want2 = d_efn2 != nullptr && g.e2 != nullptr;
	for( long long s = blockIdx.x * ( long long )SE_BLOCK + threadIdx.x; s < b.n; s += gridDim.x * ( long long )SE_BLOCK ){
		const int	w = info[ s ];
		if( rmse_info_big( w ) != BIG )
			continue;
		const long long	lo = b.off[ s ];
		const int	len = int( b.off[ s + 1 ] - lo );
		if( ( w & RMSE_INFO_INF ) || len <= 0 ){
			if( want )
				d_efn[ s ] = RME_INF;
			if( want2 )
				d_efn2[ s ] = RME2_INF;
			continue;
		}
		rme_struct_cand_t	c{ b.base + lo, { b.pair + lo * b.pair_stride, b.pair_stride }, code_s, len };
		if( len <= RMSE_CACHE )
			c.fill_cache( s_bp[ threadIdx.x ], s_bc[ threadIdx.x ] );
		if( want )
			d_efn[ s ] = rme_struct_energy<BIG>( &T, c );
		if( want2 )
			d_efn2[ s ] = rme2_struct_energy<BIG>( g.e2, c );
	}
}

}	// namespace

hipError_t struct_check( const StructBatch &b, int32_t *d_info, unsigned long long *d_bad, int wgs, int cus, hipStream_t s )
{
	if( b.n <= 0 )
		return b.n < 0 ? hipErrorInvalidValue : hipSuccess;
	// (eight workgroups a CU at most: the structures are short, the loop takes the rest)
	const int64_t	blocks = wgs > 0 ? wgs : std::min<int64_t>( ( b.n + SE_WAVES - 1 ) / SE_WAVES, int64_t( std::max( cus, 1 ) ) * 8 );
	hipLaunchKernelGGL( rma_struct_check_kernel, dim3( unsigned( blocks ) ), dim3( SE_BLOCK ), 0, s, b, d_info, d_bad );
	return hipGetLastError();
}

hipError_t struct_energies( const StructBatch &b, const int32_t *d_info, const StructTables &t, int32_t *d_efn, int32_t *d_efn2,
	int big, int wgs, int cus, hipStream_t s )
{
	if( b.n <= 0 )
		return b.n < 0 ? hipErrorInvalidValue : hipSuccess;
	const int64_t	blocks = wgs > 0 ? wgs : std::min<int64_t>( ( b.n + SE_BLOCK - 1 ) / SE_BLOCK, std::max( cus, 1 ) );
	if( big )
		hipLaunchKernelGGL( rma_struct_energy_kernel<1>, dim3( unsigned( blocks ) ), dim3( SE_BLOCK ), 0, s, b, d_info, t, d_efn, d_efn2 );
	else
		hipLaunchKernelGGL( rma_struct_energy_kernel<0>, dim3( unsigned( blocks ) ), dim3( SE_BLOCK ), 0, s, b, d_info, t, d_efn, d_efn2 );
	return hipGetLastError();
}

}	// namespace rma
