// Both ends of the MToV chunk loop on the device: what MToV/sample.py:305-400 and
// MToV/tools/dataloader_sample.py:130-247 do on the host around the four extracts, the sampler and the decode.
//   k_frames_prep    8-bit source frames -> centre crop -> bilinear resize -> v / 127.5 - 1, [B, 3, T, res, res]
//                    (resize_crop, MToV/tools/data_utils.py:73-98; with a per-frame first masked row: _crop_lower_half first)
//   k_frames_discs   integer landmark centres -> filled discs, +1 inside / -1 outside (_change_np_img_size + sample.py:325)
//   k_frames_finish  decoded frames -> the stored 8-bit frames, the 8-bit last frame and the next chunk's reference video
//                    (sample.py:385-398, 349-360)
// All three are gathers: a thread owns four neighbouring output pixels of one row, computes them from clipped source
// coordinates and writes them with one 16-byte store per float plane (12 bytes = four RGB pixels for the 8-bit outputs).  No
// input value takes part in a store address, there are no atomics and no workgroup talks to another.  At B = 1, T = 16 and
// 256 x 256 the launches have 3072 (prep) and 1024 (discs, finish) workgroups of 256 threads.
#include "plan_internal.h"

namespace {
constexpr int FR_THREADS = 256;
constexpr int FR_MAX_SIDE = 8192;        // res / canvas / source sides: keeps every in-plane index inside an int
constexpr int FR_MAX_POINTS = 1024;      // disc centres of one frame staged in LDS (8 KB)
constexpr int FR_MAX_RADIUS = 31;
constexpr int FR_FAR = 1 << 24;          // centres are clamped here when staged: still far outside any canvas, and y - cy cannot overflow

// x / 127.5 - 1 as torch computes it.  On the host that is an IEEE division; on a HIP device torch divides by a scalar by
// multiplying with its fp32 reciprocal, which differs in the last bit for 111 of the 256 byte values (RECIP: that form, the one
// MToV/sample.py:318-326 and MToVSampler.conditioning get, whose tensors are on the device when they divide).  Either way the
// subtraction is a second rounding: nothing contracts.
template <bool RECIP>
__device__ __forceinline__ float model_range(float v) {
#pragma clang fp contract(off)
    if (RECIP) {
        const float q = v * (1.0f / 127.5f);
        return q - 1.0f;
    }
    return v / 127.5f - 1.0f;
}

struct __attribute__((aligned(4))) Rgb4 {          // four RGB pixels
    uint32_t a, b, c;
};

__device__ __forceinline__ Rgb4 pack_rgb4(const uint32_t r[4], const uint32_t g[4], const uint32_t b[4]) {
    Rgb4 o;
    o.a = r[0] | g[0] << 8 | b[0] << 16 | r[1] << 24;
    o.b = g[1] | b[1] << 8 | r[2] << 16 | g[2] << 24;
    o.c = b[2] | r[3] << 8 | g[3] << 16 | b[3] << 24;
    return o;
}

// grid (ceil(res * res / 4 / 256), 3 T, B).  IDENT: h == w == res with w a multiple of 4 and a 4-byte aligned source, the four
// pixels are one 32-bit load; the general path computes the same values there (weights exactly 0 and 1).
template <bool IDENT, bool RECIP>
__global__ void __launch_bounds__(FR_THREADS) k_frames_prep(const uint8_t* __restrict__ src, const int* __restrict__ mask_start,
                                                            float* __restrict__ out, int t_in, int T, int h, int w, int res) {
#pragma clang fp contract(off)
    const int q = res >> 2;
    const int idx = blockIdx.x * FR_THREADS + threadIdx.x;
    if (idx >= res * q) return;
    const int oy = idx / q, ox = (idx - oy * q) << 2;
    const int c = blockIdx.y % 3, t = blockIdx.y / 3, b = blockIdx.z;
    const uint8_t* plane = src + ((size_t)(b * t_in + (t_in == 1 ? 0 : t)) * 3 + c) * ((size_t)h * w);
    const int ms = mask_start ? mask_start[b * T + t] : h;          // source rows >= ms read as 0
    float4 r;
    if (IDENT) {
        const uint32_t p = oy < ms ? *reinterpret_cast<const uint32_t*>(plane + (size_t)oy * w + ox) : 0u;
        r.x = model_range<RECIP>((float)(p & 255u));
        r.y = model_range<RECIP>((float)((p >> 8) & 255u));
        r.z = model_range<RECIP>((float)((p >> 16) & 255u));
        r.w = model_range<RECIP>((float)(p >> 24));
    } else {
        // centre crop to the square of the short side (data_utils.py:85-94), then ATen's upsample_bilinear2d arithmetic
        // (align_corners = False, no antialiasing): scale = float(in) / out, src = scale (dst + 0.5) - 0.5 clamped at 0,
        // i1 = i0 + (i0 < in - 1), lambda1 = src - i0
        const int S = h > w ? w : h;
        const int y_off = h > w ? (h - w) / 2 : 0, x_off = h > w ? 0 : (w - h) / 2;
        const float scale = (float)S / (float)res;
        float sy = scale * ((float)oy + 0.5f) - 0.5f;
        sy = sy < 0.0f ? 0.0f : sy;
        const int y0 = min((int)sy, S - 1), y1 = y0 + (y0 < S - 1 ? 1 : 0);
        const float ly1 = fminf(fmaxf(sy - (float)y0, 0.0f), 1.0f), ly0 = 1.0f - ly1;
        const bool live0 = y_off + y0 < ms, live1 = y_off + y1 < ms;
        const uint8_t* row0 = plane + (size_t)(y_off + y0) * w + x_off;
        const uint8_t* row1 = plane + (size_t)(y_off + y1) * w + x_off;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float sx = scale * ((float)(ox + j) + 0.5f) - 0.5f;
            sx = sx < 0.0f ? 0.0f : sx;
            const int x0 = min((int)sx, S - 1), x1 = x0 + (x0 < S - 1 ? 1 : 0);
            const float lx1 = fminf(fmaxf(sx - (float)x0, 0.0f), 1.0f), lx0 = 1.0f - lx1;
            const float a = live0 ? (float)row0[x0] : 0.0f, bb = live0 ? (float)row0[x1] : 0.0f;
            const float cc = live1 ? (float)row1[x0] : 0.0f, d = live1 ? (float)row1[x1] : 0.0f;
            v[j] = model_range<RECIP>(ly0 * (lx0 * a + lx1 * bb) + ly1 * (lx0 * cc + lx1 * d));
        }
        r = make_float4(v[0], v[1], v[2], v[3]);
    }
    *reinterpret_cast<float4*>(out + (((size_t)b * 3 + c) * T + t) * ((size_t)res * res) + (size_t)oy * res + ox) = r;
}

// grid (ceil(G * G / 4 / 256), T, B).  Row cy + dy of a disc spans cx - hw[dy + radius] .. cx + hw[dy + radius] (a negative
// half width: no pixels in that row); everything off the canvas clips because only canvas pixels are ever tested.
__global__ void __launch_bounds__(FR_THREADS) k_frames_discs(const int* __restrict__ centres, const int* __restrict__ half_width,
                                                             float* __restrict__ out, int T, int P, int radius, int G) {
    __shared__ int s_c[2 * FR_MAX_POINTS];
    __shared__ int s_hw[2 * FR_MAX_RADIUS + 1];
    const int t = blockIdx.y, b = blockIdx.z;
    const int* fc = centres + ((size_t)b * T + t) * ((size_t)P * 2);
    for (int i = threadIdx.x; i < 2 * P; i += FR_THREADS) s_c[i] = min(max(fc[i], -FR_FAR), FR_FAR);
    for (int i = threadIdx.x; i < 2 * radius + 1; i += FR_THREADS) s_hw[i] = half_width[i];
    __syncthreads();
    const int q = G >> 2;
    const int idx = blockIdx.x * FR_THREADS + threadIdx.x;
    if (idx >= G * q) return;
    const int y = idx / q, x = (idx - y * q) << 2;
    bool in0 = false, in1 = false, in2 = false, in3 = false;
    for (int p = 0; p < P; ++p) {
        const int dy = y - s_c[2 * p + 1];
        if ((unsigned)(dy + radius) > (unsigned)(2 * radius)) continue;
        const int hw = s_hw[dy + radius], dx = x - s_c[2 * p];
        in0 |= dx <= hw && dx >= -hw;
        in1 |= dx + 1 <= hw && dx + 1 >= -hw;
        in2 |= dx + 2 <= hw && dx + 2 >= -hw;
        in3 |= dx + 3 <= hw && dx + 3 >= -hw;
    }
    const float4 v = make_float4(in0 ? 1.0f : -1.0f, in1 ? 1.0f : -1.0f, in2 ? 1.0f : -1.0f, in3 ? 1.0f : -1.0f);
    const size_t plane = (size_t)G * G;
    float* o = out + ((size_t)b * 3 * T + t) * plane + (size_t)y * G + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + (size_t)c * T * plane) = v;
}

// (1 + clamp(v, -1, 1)) * 127.5 of four pixels of one channel (sample.py:385-386); a NaN reads as -1
__device__ __forceinline__ void scale_255(const float4 v, float s[4]) {
    s[0] = (1.0f + fminf(fmaxf(v.x, -1.0f), 1.0f)) * 127.5f;
    s[1] = (1.0f + fminf(fmaxf(v.y, -1.0f), 1.0f)) * 127.5f;
    s[2] = (1.0f + fminf(fmaxf(v.z, -1.0f), 1.0f)) * 127.5f;
    s[3] = (1.0f + fminf(fmaxf(v.w, -1.0f), 1.0f)) * 127.5f;
}

// grid (ceil(res * res / 4 / 256), T, B).  Every thread writes its own frame's pixels; when chaining it also reads the LAST
// frame's pixels at the same place (the T readers of a pixel share it in L2) and writes frame t of next_ref, so that the
// T-fold repeat is spread over all workgroups; the workgroups of frame T - 1 write last_u8.
__global__ void __launch_bounds__(FR_THREADS) k_frames_finish(const float* __restrict__ dec, uint8_t* __restrict__ frames_u8,
                                                              uint8_t* __restrict__ last_u8, float* __restrict__ next_ref, int T, int res) {
#pragma clang fp contract(off)
    const int q = res >> 2;
    const int idx = blockIdx.x * FR_THREADS + threadIdx.x;
    if (idx >= res * q) return;
    const int y = idx / q, x = (idx - y * q) << 2;
    const int t = blockIdx.y, b = blockIdx.z;
    const size_t plane = (size_t)res * res, at = (size_t)y * res + x;
    {
        const float* f = dec + (size_t)(b * T + t) * 3 * plane + at;
        float s[4];
        uint32_t u[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            scale_255(*reinterpret_cast<const float4*>(f + c * plane), s);
#pragma unroll
            for (int j = 0; j < 4; ++j) u[c][j] = (uint32_t)s[j];              // truncation: fake.type(torch.uint8), sample.py:402
        }
        *reinterpret_cast<Rgb4*>(frames_u8 + ((size_t)(b * T + t) * plane + at) * 3) = pack_rgb4(u[0], u[1], u[2]);
    }
    if (next_ref == nullptr) return;
    const float* l = dec + (size_t)(b * T + T - 1) * 3 * plane + at;
    float s[4];
    uint32_t u[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        scale_255(*reinterpret_cast<const float4*>(l + c * plane), s);
        float4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) u[c][j] = (uint32_t)fminf(fmaxf(rintf(s[j]), 0.0f), 255.0f);   // np.rint (half to even), clip: sample.py:397
        // ToTensor's / 255, then * 2 - 1 (sample.py:352-353)
        r.x = (float)u[c][0] / 255.0f * 2.0f - 1.0f;
        r.y = (float)u[c][1] / 255.0f * 2.0f - 1.0f;
        r.z = (float)u[c][2] / 255.0f * 2.0f - 1.0f;
        r.w = (float)u[c][3] / 255.0f * 2.0f - 1.0f;
        *reinterpret_cast<float4*>(next_ref + (((size_t)b * 3 + c) * T + t) * plane + at) = r;
    }
    if (t == T - 1) *reinterpret_cast<Rgb4*>(last_u8 + ((size_t)b * plane + at) * 3) = pack_rgb4(u[0], u[1], u[2]);
}

bool aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
bool count_ok(int n) { return n >= 1 && n <= 4096; }      // grid y / z and the int products b * T + t
bool side_ok(int n) { return n >= 4 && n <= FR_MAX_SIDE && n % 4 == 0; }
unsigned row_blocks(int side) { return (unsigned)((side * (side >> 2) + FR_THREADS - 1) / FR_THREADS); }
}  // namespace

extern "C" {

int mtv_frames_prep(const uint8_t* src, const int32_t* mask_start, float* out, int batch, int frames_in, int frames, int height,
                    int width, int res, int division, void* stream) {
    if (!src || !out) return fail(MTV_ERR_INVALID, "mtv_frames_prep: null tensor pointer");
    if (!count_ok(batch) || !count_ok(frames)) return fail(MTV_ERR_INVALID, "mtv_frames_prep: batch and frames must be 1..4096");
    if (frames_in != 1 && frames_in != frames) return fail(MTV_ERR_INVALID, "mtv_frames_prep: frames_in must be 1 (broadcast) or frames");
    if (height < 1 || width < 1 || height > FR_MAX_SIDE || width > FR_MAX_SIDE) return fail(MTV_ERR_INVALID, "mtv_frames_prep: source sides must be 1..8192");
    if (!side_ok(res)) return fail(MTV_ERR_INVALID, "mtv_frames_prep: res must be a multiple of 4 in 4..8192");
    if (!aligned(out, 16)) return fail(MTV_ERR_INVALID, "mtv_frames_prep: out must be 16-byte aligned");
    if (mask_start && !aligned(mask_start, 4)) return fail(MTV_ERR_INVALID, "mtv_frames_prep: mask_start must be 4-byte aligned");
    if (division != MTV_FRAMES_DIV_IEEE && division != MTV_FRAMES_DIV_RECIPROCAL)
        return fail(MTV_ERR_INVALID, "mtv_frames_prep: division must be MTV_FRAMES_DIV_IEEE or MTV_FRAMES_DIV_RECIPROCAL");
    const dim3 grid(row_blocks(res), (unsigned)(3 * frames), (unsigned)batch);
    hipStream_t s = (hipStream_t)stream;
    const bool ident = height == res && width == res && aligned(src, 4), recip = division == MTV_FRAMES_DIV_RECIPROCAL;
    auto kernel = ident ? (recip ? k_frames_prep<true, true> : k_frames_prep<true, false>)
                        : (recip ? k_frames_prep<false, true> : k_frames_prep<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(FR_THREADS), 0, s, src, mask_start, out, frames_in, frames, height, width, res);
    HIPCHK(hipGetLastError());
    return MTV_OK;
}

int mtv_frames_discs(const int32_t* centres, const int32_t* half_width, float* out, int batch, int frames, int points, int radius,
                     int canvas, void* stream) {
    if (!centres || !half_width || !out) return fail(MTV_ERR_INVALID, "mtv_frames_discs: null tensor pointer");
    if (!count_ok(batch) || !count_ok(frames)) return fail(MTV_ERR_INVALID, "mtv_frames_discs: batch and frames must be 1..4096");
    if (points < 1 || points > FR_MAX_POINTS) return fail(MTV_ERR_INVALID, "mtv_frames_discs: points must be 1..1024");
    if (radius < 0 || radius > FR_MAX_RADIUS) return fail(MTV_ERR_INVALID, "mtv_frames_discs: radius must be 0..31");
    if (!side_ok(canvas)) return fail(MTV_ERR_INVALID, "mtv_frames_discs: canvas must be a multiple of 4 in 4..8192");
    if (!aligned(out, 16) || !aligned(centres, 4) || !aligned(half_width, 4)) return fail(MTV_ERR_INVALID, "mtv_frames_discs: out must be 16-byte, the integer tables 4-byte aligned");
    hipLaunchKernelGGL(k_frames_discs, dim3(row_blocks(canvas), (unsigned)frames, (unsigned)batch), dim3(FR_THREADS), 0, (hipStream_t)stream,
                       centres, half_width, out, frames, points, radius, canvas);
    HIPCHK(hipGetLastError());
    return MTV_OK;
}

int mtv_frames_finish(const float* decoded, uint8_t* frames_u8, uint8_t* last_u8, float* next_ref, int batch, int frames, int res,
                      void* stream) {
    if (!decoded || !frames_u8) return fail(MTV_ERR_INVALID, "mtv_frames_finish: null tensor pointer");
    if ((last_u8 == nullptr) != (next_ref == nullptr)) return fail(MTV_ERR_INVALID, "mtv_frames_finish: last_u8 and next_ref are requested together or not at all");
    if (!count_ok(batch) || !count_ok(frames)) return fail(MTV_ERR_INVALID, "mtv_frames_finish: batch and frames must be 1..4096");
    if (!side_ok(res)) return fail(MTV_ERR_INVALID, "mtv_frames_finish: res must be a multiple of 4 in 4..8192");
    if (!aligned(decoded, 16) || !aligned(frames_u8, 4) || (next_ref && (!aligned(next_ref, 16) || !aligned(last_u8, 4))))
        return fail(MTV_ERR_INVALID, "mtv_frames_finish: float tensors must be 16-byte, 8-bit tensors 4-byte aligned");
    hipLaunchKernelGGL(k_frames_finish, dim3(row_blocks(res), (unsigned)frames, (unsigned)batch), dim3(FR_THREADS), 0, (hipStream_t)stream,
                       decoded, frames_u8, last_u8, next_ref, frames, res);
    HIPCHK(hipGetLastError());
    return MTV_OK;
}

}  // extern "C"
