// JPEG decode split between host and device (include/ssd_hip.h has the contract and the arithmetic).
//   ssd_jpeg_info, ssd_jpeg_entropy_decode   host only: jpeg_host.h (marker parsing, Huffman), no HIP call
//   ssd_jpeg_reconstruct                     k_jpeg_idct: dequantise + 8x8 integer IDCT, one block per lane, into padded uint8
//                                            sample planes; k_jpeg_rgb: chroma upsampling + colour conversion, one pixel per
//                                            lane, interleaved RGB straight into the arena ssd_image_resize_prep reads
// One launch pair serves a ragged batch: blockIdx.y is the image, blockIdx.x strides over its blocks / pixels.  The records
// live on the device, so the kernels (not the host) check that a record's planes and destination lie inside the buffers; a
// record that fails writes nothing.  All arithmetic is done on unsigned words (wrapping) and shifted as signed: coefficients
// no encoder can produce give unspecified samples, never undefined behaviour or a stray access.
#include "common.h"
#include "jpeg_host.h"

namespace {

constexpr int IDCT_GRID_X = 64;       // x 256 lanes: 16 384 blocks per stride (a VGA 4:2:0 image has 7 200)
constexpr int RGB_GRID_X = 128;       // x 256 lanes: 32 768 pixels per stride

struct Rec {                          // the fields of one record a kernel needs, validated
    int W, H, kind, ncomp, cw, ch;    // cw, ch: chroma plane extent after cropping (= W, H for 4:4:4)
    int bw[3], bh[3];
    long long off[3];
    bool ok;
};

__device__ __forceinline__ Rec load_rec(const int* __restrict__ r, long long total_coef) {
    Rec d;
    d.W = r[SSD_JPEG_WIDTH];
    d.H = r[SSD_JPEG_HEIGHT];
    d.kind = r[SSD_JPEG_KIND];
    d.ok = d.W >= 1 && d.W <= 65535 && d.H >= 1 && d.H <= 65535 && d.kind >= SSD_JPEG_GREY && d.kind <= SSD_JPEG_420;
    d.ncomp = d.kind == SSD_JPEG_GREY ? 1 : 3;
    d.cw = (d.kind == SSD_JPEG_422 || d.kind == SSD_JPEG_420) ? (d.W + 1) >> 1 : d.W;
    d.ch = d.kind == SSD_JPEG_420 ? (d.H + 1) >> 1 : d.H;
    for (int c = 0; c < 3; ++c) {
        d.bw[c] = c < d.ncomp ? r[SSD_JPEG_BLOCKS_W + c] : 0;
        d.bh[c] = c < d.ncomp ? r[SSD_JPEG_BLOCKS_H + c] : 0;
        d.off[c] = c < d.ncomp ? (long long)r[SSD_JPEG_COEF_OFF + c] : 0;
        if (c < d.ncomp) {
            const int need_w = c ? d.cw : d.W, need_h = c ? d.ch : d.H;
            d.ok = d.ok && d.bw[c] >= 1 && d.bw[c] <= 16384 && d.bh[c] >= 1 && d.bh[c] <= 16384 && d.bw[c] * 8 >= need_w &&
                   d.bh[c] * 8 >= need_h && d.off[c] >= 0 && (d.off[c] & 63) == 0 &&
                   d.off[c] + 64LL * d.bw[c] * d.bh[c] <= total_coef;
        }
    }
    return d;
}

__device__ __forceinline__ int ds(unsigned x, int n) { return (int)(x + (1u << (n - 1))) >> n; }

// one pass of the scaled integer IDCT over d[0..7]; out = DS(., shift)
__device__ __forceinline__ void idct8(const unsigned* d, int* out, int shift) {
    unsigned z1 = (d[2] + d[6]) * 4433u;
    const unsigned t2 = z1 - d[6] * 15137u, t3 = z1 + d[2] * 6270u;
    const unsigned t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
    const unsigned t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    unsigned o0 = d[7], o1 = d[5], o2 = d[3], o3 = d[1];
    z1 = o0 + o3;
    unsigned z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const unsigned z5 = (z3 + z4) * 9633u;
    o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
    z1 *= (unsigned)-7373; z2 *= (unsigned)-20995;
    z3 = z3 * (unsigned)-16069 + z5;
    z4 = z4 * (unsigned)-3196 + z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    out[0] = ds(t10 + o3, shift); out[7] = ds(t10 - o3, shift);
    out[1] = ds(t11 + o2, shift); out[6] = ds(t11 - o2, shift);
    out[2] = ds(t12 + o1, shift); out[5] = ds(t12 - o1, shift);
    out[3] = ds(t13 + o0, shift); out[4] = ds(t13 - o0, shift);
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(256) void k_jpeg_idct(const short* __restrict__ coef, const int* __restrict__ desc,
                                                   unsigned char* __restrict__ planes, long long total_coef) {
    __shared__ int qt[192];
    const int* r = desc + (long long)blockIdx.y * SSD_JPEG_REC_WORDS;
    const Rec d = load_rec(r, total_coef);
    if (!d.ok) return;                                                       // uniform over the workgroup
    const int n0 = d.bw[0] * d.bh[0], n1 = d.bw[1] * d.bh[1], n2 = d.bw[2] * d.bh[2];
    const long long nblk = (long long)n0 + n1 + n2;
    if ((long long)blockIdx.x * 256 >= nblk) return;
    if (threadIdx.x < 64 * d.ncomp) qt[threadIdx.x] = r[SSD_JPEG_QT + threadIdx.x];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nblk; i += (long long)IDCT_GRID_X * 256) {
        int c = 0;
        long long bi = i;
        if (bi >= n0) { bi -= n0; c = 1; if (bi >= n1) { bi -= n1; c = 2; } }
        const int bwc = c == 0 ? d.bw[0] : (c == 1 ? d.bw[1] : d.bw[2]);       // (selects, not indexing: Rec stays in registers)
        const long long offc = c == 0 ? d.off[0] : (c == 1 ? d.off[1] : d.off[2]);
        const int by = (int)(bi / bwc), bx = (int)(bi - (long long)by * bwc);
        const uint4* src = reinterpret_cast<const uint4*>(coef + offc + 64 * bi);         // 128-byte aligned
        const int* q = qt + 64 * c;
        int ws[64];
        unsigned col[8][8];                                                  // [row k][column]: dequantised
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint4 v = src[k];
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                col[k][2 * j] = (unsigned)(int)(short)(w[j] & 0xffffu) * (unsigned)q[8 * k + 2 * j];
                col[k][2 * j + 1] = (unsigned)(int)(short)(w[j] >> 16) * (unsigned)q[8 * k + 2 * j + 1];
            }
        }
#pragma unroll
        for (int x = 0; x < 8; ++x) {                                        // columns, DS(., 11)
            unsigned in[8];
            int out[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) in[k] = col[k][x];
            idct8(in, out, 11);
#pragma unroll
            for (int k = 0; k < 8; ++k) ws[8 * k + x] = out[k];
        }
        unsigned char* dst = planes + offc + ((long long)by * 8) * (bwc * 8) + bx * 8;
#pragma unroll
        for (int y = 0; y < 8; ++y) {                                        // rows, DS(., 18), + 128, clamp
            unsigned in[8];
            int out[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) in[k] = (unsigned)ws[8 * y + k];
            idct8(in, out, 18);
            unsigned lo = 0, hi = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lo |= clamp255(out[k] + 128) << (8 * k);
                hi |= clamp255(out[k + 4] + 128) << (8 * k);
            }
            *reinterpret_cast<uint2*>(dst + (long long)y * (bwc * 8)) = make_uint2(lo, hi);       // 8-byte aligned
        }
    }
}

__global__ __launch_bounds__(256) void k_jpeg_rgb(const unsigned char* __restrict__ planes, const int* __restrict__ desc,
                                                  unsigned char* __restrict__ dst, const long long* __restrict__ dst_off,
                                                  long long dst_bytes, long long total_coef) {
    const Rec d = load_rec(desc + (long long)blockIdx.y * SSD_JPEG_REC_WORDS, total_coef);
    if (!d.ok) return;
    const long long npix = (long long)d.W * d.H, base = dst_off[blockIdx.y];
    if (base < 0 || base > dst_bytes || 3 * npix > dst_bytes - base) return;
    const unsigned char* py = planes + d.off[0];
    const unsigned char* pcb = planes + d.off[1];
    const unsigned char* pcr = planes + d.off[2];
    const int sy = d.bw[0] * 8, sc = d.bw[1] * 8, sr = d.bw[2] * 8;
    unsigned char* out = dst + base;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)RGB_GRID_X * 256) {
        const int y = (int)(i / d.W), x = (int)(i - (long long)y * d.W);
        const int Y = py[(long long)y * sy + x];
        int R = Y, G = Y, B = Y;
        if (d.kind != SSD_JPEG_GREY) {
            int cb, cr;
            if (d.kind == SSD_JPEG_444) {
                cb = pcb[(long long)y * sc + x];
                cr = pcr[(long long)y * sr + x];
            } else {
                const int ci = x >> 1;
                const int lo = ci > 0 ? ci - 1 : 0, hi = ci + 1 < d.cw ? ci + 1 : d.cw - 1;
                const int cn = (x & 1) ? hi : lo;                            // the horizontal neighbour of this output column
                const bool edge = cn == ci;                                  // first / last output column
                if (d.kind == SSD_JPEG_422) {
                    const unsigned char* b0 = pcb + (long long)y * sc;
                    const unsigned char* r0 = pcr + (long long)y * sr;
                    if (d.cw <= 2 || edge) {
                        cb = b0[ci];
                        cr = r0[ci];
                    } else {
                        const int rnd = (x & 1) ? 2 : 1;
                        cb = (3 * b0[ci] + b0[cn] + rnd) >> 2;
                        cr = (3 * r0[ci] + r0[cn] + rnd) >> 2;
                    }
                } else {
                    const int cj = y >> 1;
                    const int jn = (y & 1) ? (cj + 1 < d.ch ? cj + 1 : d.ch - 1) : (cj > 0 ? cj - 1 : 0);
                    const unsigned char* b0 = pcb + (long long)cj * sc;
                    const unsigned char* b1 = pcb + (long long)jn * sc;
                    const unsigned char* r0 = pcr + (long long)cj * sr;
                    const unsigned char* r1 = pcr + (long long)jn * sr;
                    if (d.cw <= 2) {
                        cb = b0[ci];
                        cr = r0[ci];
                    } else {
                        const int rnd = (x & 1) ? 7 : 8;
                        const int vb = 3 * b0[ci] + b1[ci], vr = 3 * r0[ci] + r1[ci];
                        if (edge) {
                            cb = (4 * vb + rnd) >> 4;
                            cr = (4 * vr + rnd) >> 4;
                        } else {
                            cb = (3 * vb + 3 * b0[cn] + b1[cn] + rnd) >> 4;
                            cr = (3 * vr + 3 * r0[cn] + r1[cn] + rnd) >> 4;
                        }
                    }
                }
            }
            cb -= 128;
            cr -= 128;
            R = Y + ((91881 * cr + 32768) >> 16);
            G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
            B = Y + ((116130 * cb + 32768) >> 16);
        }
        unsigned char* o = out + 3 * i;
        o[0] = (unsigned char)clamp255(R);
        o[1] = (unsigned char)clamp255(G);
        o[2] = (unsigned char)clamp255(B);
    }
}

}  // namespace

extern "C" {

int ssd_jpeg_info(const void* data, size_t n, int32_t* rec) { return ssd_jpeg::info(data, n, rec); }

int ssd_jpeg_entropy_decode(const void* data, size_t n, int16_t* coef, size_t capacity, int32_t* rec) {
    return ssd_jpeg::entropy_decode(data, n, coef, capacity, rec);
}

size_t ssd_jpeg_reconstruct_workspace_bytes(long long total_coef) { return total_coef > 0 ? (size_t)total_coef : 0; }

int ssd_jpeg_reconstruct(const int16_t* coef, const int32_t* desc, int B, uint8_t* dst, const int64_t* dst_off,
                         long long dst_bytes, void* scratch, size_t scratch_bytes, long long total_coef, void* stream) {
    if (!coef || !desc || !dst || !dst_off || B <= 0 || B > 65535 || total_coef <= 0 || (total_coef & 63) || dst_bytes <= 0)
        return SSD_ERR_VALUE;
    if (((uintptr_t)coef & 15) || ((uintptr_t)desc & 3) || ((uintptr_t)dst_off & 7) || ((uintptr_t)scratch & 15)) return SSD_ERR_VALUE;
    if (!scratch || scratch_bytes < ssd_jpeg_reconstruct_workspace_bytes(total_coef)) return SSD_ERR_WORKSPACE;
    hipLaunchKernelGGL(k_jpeg_idct, dim3(IDCT_GRID_X, (unsigned)B), dim3(256), 0, (hipStream_t)stream, coef, desc,
                       static_cast<unsigned char*>(scratch), total_coef);
    if (hipGetLastError() != hipSuccess) return SSD_ERR_LAUNCH;
    hipLaunchKernelGGL(k_jpeg_rgb, dim3(RGB_GRID_X, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(scratch), desc, dst, reinterpret_cast<const long long*>(dst_off),
                       dst_bytes, total_coef);
    return ssd_launch_status();
}

}  // extern "C"
