// meao_k_linear.hip -- the kernels that read linear view-space depth (MEAO_DEPTH_LINEAR_F32 / _F16): the stand-alone downsample
// pass, the full-resolution upsample (64 x 64 and small tiles) and LinearDepth for debug id 1.  The same device functions as
// meao_k_downsample.hip / meao_k_upsample.hip / meao_k_misc.hip with LINEAR set: decode and Linearize become "widen, multiply by
// s, far-plane select" (linearize_view; s in the zp0 field).  They address caller memory through the pitch fields (PITCHED), so
// one instance serves packed (pitch = width) and pitched calls.  Units of their own, so that the other kernels compile exactly
// as they would without them.
#include "meao_dev_downsample.hpp"
#include "meao_dev_upsample.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

template <bool VEC, int DIV, int ROWS>
__global__ __launch_bounds__(kThreads) void downsample_linear_kernel(const DownsampleArgs a)
{
    downsample_tile<VEC, DIV, ROWS, true, true>(a, blockIdx.x, blockIdx.z);
}

// F32: f32 texels, else f16 (8-byte loads of four texels where vec_ok)
template <int AOFMT, bool RTNE, int DIV, bool F32>
__global__ __launch_bounds__(kThreads, 7) void upsample_final_linear_kernel(const UpsampleArgs a, const HiDepthArgs hi)
{
    typedef FinalForm<ups_tile_h(true), RawDepth(F32), Rows::Pitched, DepthKind::Linear> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, NoHook(), &hi);
}

template <int AOFMT, bool RTNE, int DIV, bool F32>
__global__ __launch_bounds__(kThreads) void upsample_final_small_linear_kernel(const UpsampleArgs a, const HiDepthArgs hi)
{
    typedef FinalForm<kUpsTileHSmall, RawDepth(F32), Rows::Pitched, DepthKind::Linear> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, NoHook(), &hi);
}

// LinearDepth (debug id 1) of a linear frame: f16(linearize_view(z)), packed frame
template <bool RTNE>
__global__ __launch_bounds__(kThreads) void linear_depth_view_kernel(const LinearDepthArgs a)
{
    const int format = linear_texel_format(a.depth_format);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < a.pixels; i += static_cast<int64_t>(gridDim.x) * kThreads)
        a.dst[i] = f32_to_f16_bits<RTNE>(linearize_view(raw_depth_texel(a.depth, format, static_cast<size_t>(i)), a.zp0));
}

}  // namespace

// (every stride of the blocks is set: a packed side carries its packed row)
hipError_t launch_downsample_linear(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf)
{
    if (!linear_depth(a.depth_format) || !rows_per_lane_valid(a) || !depth_stride_set(a)) return hipErrorInvalidValue;
    if (pf) return launch_downsample_linear_frames(a, frames, s, pf);
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    return for_downsample_variant(a, [&](auto v) { downsample_linear_kernel<v.kVec, v.kDiv, v.kRows><<<grid, dim3(kThreads), 0, s>>>(a); });
}

hipError_t launch_upsample_final_linear(const UpsampleArgs &a, const HiDepthArgs &hi, int ao_format, int frames, hipStream_t s,
                                        const UpsampleArgs *pf, const HiDepthArgs *pf_hi)
{
    if (!linear_depth(hi.depth_format) || !final_strides_set(a)) return hipErrorInvalidValue;
    if (pf) return launch_upsample_final_linear_frames(a, hi, ao_format, frames, s, pf, pf_hi);
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames), block(kThreads);
    return for_column(ao_format, a, [&](auto c) {
        for_final_variant<MEAO_DEPTH_LINEAR_F32>(a, hi, [&](auto v) {
            if constexpr (v.kSmall) upsample_final_small_linear_kernel<c.kAoFmt, c.kRtne, c.kDiv, v.kF32><<<grid, block, 0, s>>>(a, hi);
            else upsample_final_linear_kernel<c.kAoFmt, c.kRtne, c.kDiv, v.kF32><<<grid, block, 0, s>>>(a, hi);
        });
    });
}

hipError_t launch_linear_depth_view(const LinearDepthArgs &a, hipStream_t s)
{
    if (!linear_depth(a.depth_format)) return hipErrorInvalidValue;
    const dim3 grid(static_cast<int>(std::min<int64_t>((a.pixels + kThreads - 1) / kThreads, 256 * 32))), block(kThreads);
    if (a.f16_rtne) linear_depth_view_kernel<true><<<grid, block, 0, s>>>(a);
    else linear_depth_view_kernel<false><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace meao
