// jpeg.hip -- baseline JPEG encoder on the device, byte-exact with Pillow's default save (gfx950).
//
// The reference's compressibility reward (adv_grpo/rewards.py:13-35) copies every image to the host and saves it with
// Pillow (libjpeg-turbo) as a quality-95 JPEG only to read the byte count.  The encoder below computes the same file on
// the device: baseline sequential, 4:2:0, the Annex K Huffman tables, no restart markers, the JFIF header Pillow writes.
// All arithmetic is integer and follows the JPEG standard (ITU-T T.81) and the IJG conventions Pillow's library uses:
//
//   quantise   (x*255).round().clamp(0,255) in the input's dtype (bf16: the product rounded to bf16 first)
//   colour     Y/Cb/Cr in 16-bit fixed point, FIX(x) = (int)(x*65536 + 0.5)
//   chroma     2x2 box, (a+b+c+d + bias) >> 2, bias 1 on even output columns and 2 on odd ones
//   DCT        the accurate integer DCT (Loeffler-Ligtenberg-Moschytz; CONST_BITS 13, PASS1_BITS 2), rows then columns;
//              the output is 8x the orthonormal DCT
//   quant      divisor d = 8*q[k]: sign(c) * ((|c| + d/2) / d)
//
// Kernels (per call):
//   1. dct     one wave per 8x8 block (blocks in MCU order Y0 Y1 Y2 Y3 Cb Cr): pixels -> level-shifted samples -> DCT ->
//              quantised zig-zag coefficients (int16), and the bit count of the block's AC part (ballot of the nonzero mask)
//   2. scan    one workgroup per image: adds each block's DC-difference bits, prefix-sums the block bit counts into bit
//              offsets, zeroes the bitstream words each block shares with a neighbour
//   3. emit    one wave per block: each lane's complete bit string (<= 3 ZRL + code + magnitude + EOB <= 63 bits) in one
//              64-bit value, a wave prefix sum places it; the block's words are assembled in LDS, interior words stored
//              plainly, the two boundary words OR-ed in with integer atomics (order-independent: same bytes every run)
//   4. count   0xFF bytes per 4 KB chunk of each image's entropy-coded segment (final byte padded with 1-bits)
//   5. finish  one workgroup per image: chunk prefix of the 0xFF counts, sizes[n] = header + bytes + stuffed zeros + EOI;
//              with files: the header and the EOI marker
//   6. scatter (files only) every entropy-coded byte to its stuffed position, 0x00 after each 0xFF
#include "common.hpp"

namespace advgrpo {
namespace jpg {

constexpr int HEADER_BYTES = 623;
// a block codes at most 22 DC bits (11-bit code + 11 magnitude bits), 63 AC coefficients of <= 16 + 10 bits, <= 3 ZRL codes of
// <= 11 bits (a run of 16 zeros each; 62 positions) and one 4-bit EOB; the coding below clamps the sizes so it cannot exceed it
constexpr int64_t MAX_BLOCK_BITS = 22 + 63 * 26 + 3 * 11 + 4;
constexpr int CHUNK = 4096;   // bytes of entropy-coded segment per workgroup in the 0xFF count / scatter passes
constexpr int WAVES = 4;      // blocks (waves) per workgroup in the dct / emit passes

#define JPEG_ZIGZAG                                                                                                            \
    { 0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 }
// ITU-T T.81 Annex K.1 (natural order)
constexpr uint8_t kLumaBase[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                   14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                   18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kChromaBase[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr uint8_t kZigzagHost[64] = JPEG_ZIGZAG;
__constant__ uint8_t c_zigzag[64] = JPEG_ZIGZAG;

// ITU-T T.81 Annex K.3: code counts per length 1..16 and symbols, DC / AC x luminance / chrominance
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// canonical codes of a (bits, vals) table (T.81 Annex C): symbol -> code | length << 16
struct HuffCodes {
    uint32_t ehuf[256];
};
constexpr HuffCodes make_codes(const uint8_t (&bits)[16], const uint8_t* vals) {
    HuffCodes h{};
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k) h.ehuf[vals[k]] = code++ | ((uint32_t)l << 16);
        code <<= 1;
    }
    return h;
}
struct HuffTables {
    HuffCodes dc[2], ac[2];   // [0] luminance, [1] chrominance
};
constexpr HuffTables make_tables() {
    return HuffTables{{make_codes(kDcLumaBits, kDcVals), make_codes(kDcChromaBits, kDcVals)},
                      {make_codes(kAcLumaBits, kAcLumaVals), make_codes(kAcChromaBits, kAcChromaVals)}};
}
__constant__ HuffTables c_huff = make_tables();

struct QuantTables {
    uint16_t q[2][64];   // natural order; [0] luminance, [1] chrominance
};
struct Header {
    uint8_t b[HEADER_BYTES + 1];
};

// ---- pixels
__device__ inline int load_u8(const void* img, int dt, int64_t i) {
    if (dt == ADVGRPO_U8) return reinterpret_cast<const uint8_t*>(img)[i];
    float v = (dt == ADVGRPO_BF16 ? bf2f(reinterpret_cast<const bf16_t*>(img)[i]) : reinterpret_cast<const float*>(img)[i]) * 255.0f;
    if (dt == ADVGRPO_BF16) v = round_bf16(v);   // the product is a bf16 torch op when the images are bf16
    return (int)fminf(fmaxf(rintf(v), 0.f), 255.f);
}
constexpr int FIX16(double x) { return (int)(x * 65536.0 + 0.5); }
__device__ inline void load_rgb(const void* img, int dt, int layout, int H, int W, int n, int y, int x, int& r, int& g, int& b) {
    if (layout == ADVGRPO_JPEG_NHWC) {
        const int64_t i = (((int64_t)n * H + y) * W + x) * 3;
        r = load_u8(img, dt, i); g = load_u8(img, dt, i + 1); b = load_u8(img, dt, i + 2);
    } else {
        const int64_t plane = (int64_t)H * W, i = (int64_t)n * 3 * plane + (int64_t)y * W + x;
        r = load_u8(img, dt, i); g = load_u8(img, dt, i + plane); b = load_u8(img, dt, i + 2 * plane);
    }
}
__device__ inline int rgb_to_y(int r, int g, int b) { return (FIX16(0.299) * r + FIX16(0.587) * g + FIX16(0.114) * b + (1 << 15)) >> 16; }
__device__ inline int rgb_to_cb(int r, int g, int b) {
    return (-FIX16(0.16874) * r - FIX16(0.33126) * g + FIX16(0.5) * b + (128 << 16) + (1 << 15) - 1) >> 16;
}
__device__ inline int rgb_to_cr(int r, int g, int b) {
    return (FIX16(0.5) * r - FIX16(0.41869) * g - FIX16(0.08131) * b + (128 << 16) + (1 << 15) - 1) >> 16;
}

// ---- accurate integer forward DCT, one 8-point pass (PASS 1: rows, scaled up by 2^PASS1_BITS; PASS 2: columns)
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int FIX13(double x) { return (int)(x * 8192.0 + 0.5); }
__device__ inline int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
template <int PASS>
__device__ inline void fdct8(int* d, int s) {
    constexpr int SH = PASS == 1 ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    const int t0 = d[0] + d[7 * s], t7 = d[0] - d[7 * s], t1 = d[s] + d[6 * s], t6 = d[s] - d[6 * s];
    const int t2 = d[2 * s] + d[5 * s], t5 = d[2 * s] - d[5 * s], t3 = d[3 * s] + d[4 * s], t4 = d[3 * s] - d[4 * s];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (PASS == 1) {
        d[0] = (t10 + t11) * (1 << PASS1_BITS);
        d[4 * s] = (t10 - t11) * (1 << PASS1_BITS);
    } else {
        d[0] = descale(t10 + t11, PASS1_BITS);
        d[4 * s] = descale(t10 - t11, PASS1_BITS);
    }
    const int z1e = (t12 + t13) * FIX13(0.541196100);
    d[2 * s] = descale(z1e + t13 * FIX13(0.765366865), SH);
    d[6 * s] = descale(z1e - t12 * FIX13(1.847759065), SH);
    // odd part
    const int z5 = (t4 + t6 + t5 + t7) * FIX13(1.175875602);
    const int z1 = (t4 + t7) * -FIX13(0.899976223), z2 = (t5 + t6) * -FIX13(2.562915447);
    const int z3 = (t4 + t6) * -FIX13(1.961570560) + z5, z4 = (t5 + t7) * -FIX13(0.390180644) + z5;
    d[7 * s] = descale(t4 * FIX13(0.298631336) + z1 + z3, SH);
    d[5 * s] = descale(t5 * FIX13(2.053119869) + z2 + z4, SH);
    d[3 * s] = descale(t6 * FIX13(3.072711026) + z2 + z3, SH);
    d[s] = descale(t7 * FIX13(1.501321110) + z1 + z4, SH);
}

// ---- entropy coding
__device__ inline int category(int v) { return v ? 32 - __builtin_clz((unsigned)(v < 0 ? -v : v)) : 0; }
__device__ inline void put(uint64_t& acc, int& len, uint32_t e) {   // append a Huffman code (code | length << 16)
    const int l = e >> 16;
    acc = (acc << l) | (e & 0xffff);
    len += l;
}
__device__ inline void put_value(uint64_t& acc, int& len, int v, int s) {   // the s magnitude bits of v (T.81 F.1.2.1)
    acc = (acc << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1));
    len += s;
}
// The bit string lane k of a block's wave contributes, MSB-first in the low `len` bits: the DC difference (k == 0), or the
// ZRL codes, run/size code and magnitude of nonzero AC coefficient k; EOB after the last nonzero coefficient when the block
// ends in zeros.  mask: nonzero AC coefficients (bit k, k >= 1).  <= 63 bits: 3 * 11 + 16 + 10 + 4.
__device__ inline uint64_t lane_bits(int k, int v, uint64_t mask, int dcdiff, int comp, int& len) {
    uint64_t acc = 0;
    len = 0;
    const HuffCodes& ac = c_huff.ac[comp];
    if (k == 0) {
        const int s = min(category(dcdiff), 11);
        put(acc, len, c_huff.dc[comp].ehuf[s]);
        put_value(acc, len, dcdiff, s);
        if (mask == 0) put(acc, len, ac.ehuf[0x00]);
        return acc;
    }
    if (v == 0) return 0;
    const uint64_t below = mask & ((1ull << k) - 1);
    int run = k - 1 - (below ? 63 - __builtin_clzll(below) : 0);
    for (; run >= 16; run -= 16) put(acc, len, ac.ehuf[0xf0]);
    const int s = min(category(v), 10);
    put(acc, len, ac.ehuf[(run << 4) | s]);
    put_value(acc, len, v, s);
    if (k < 63 && (mask >> (k + 1)) == 0) put(acc, len, ac.ehuf[0x00]);
    return acc;
}
// block b of an image in MCU order -> component (0 Y, 1 Cb, 2 Cr) and the block whose DC predicts it (-1: none)
__device__ inline int block_comp(int b) { const int j = b % 6; return j < 4 ? 0 : j - 3; }
__device__ inline int dc_pred_block(int b) {
    const int j = b % 6;
    if (j >= 1 && j <= 3) return b - 1;
    if (b < 6) return -1;
    return j == 0 ? b - 3 : b - 6;
}
__device__ inline int dc_diff(const int16_t* coef_img, int b) {
    const int p = dc_pred_block(b);
    return coef_img[(int64_t)b * 64] - (p < 0 ? 0 : coef_img[(int64_t)p * 64]);
}

__device__ inline int wave_sum_int(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- 1. pixels -> quantised zig-zag coefficients + AC bit count, one wave per block
__global__ __launch_bounds__(64 * WAVES) void jpeg_dct_kernel(const void* __restrict__ img, int dt, int layout, int H, int W,
                                                              int nblk, int64_t total, QuantTables qt,
                                                              int16_t* __restrict__ coef, int* __restrict__ blen) {
    __shared__ int sm[WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * WAVES + w;
    const bool live = g < total;
    const int n = live ? (int)(g / nblk) : 0, b = live ? (int)(g % nblk) : 0;
    const int mcu = b / 6, j = b % 6, mw = W / 16;
    const int my = mcu / mw, mx = mcu % mw, r = lane >> 3, c = lane & 7;
    int sample;
    if (j < 4) {
        int R, G, B;
        load_rgb(img, dt, layout, H, W, n, my * 16 + (j >> 1) * 8 + r, mx * 16 + (j & 1) * 8 + c, R, G, B);
        sample = rgb_to_y(R, G, B);
    } else {
        int sum = 0;
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                int R, G, B;
                load_rgb(img, dt, layout, H, W, n, my * 16 + 2 * r + dy, mx * 16 + 2 * c + dx, R, G, B);
                sum += j == 4 ? rgb_to_cb(R, G, B) : rgb_to_cr(R, G, B);
            }
        sample = (sum + 1 + (c & 1)) >> 2;   // output column parity == c parity (blocks start on even columns)
    }
    sm[w][lane] = sample - 128;
    __syncthreads();
    if (lane < 8) fdct8<1>(&sm[w][lane * 8], 1);
    __syncthreads();
    if (lane < 8) fdct8<2>(&sm[w][lane], 8);
    __syncthreads();
    const int comp = j < 4 ? 0 : j - 3;
    const int nat = c_zigzag[lane];
    const int cv = sm[w][nat], d = qt.q[comp ? 1 : 0][nat] << 3;
    const int a = ((cv < 0 ? -cv : cv) + (d >> 1)) / d;
    const int v = cv < 0 ? -a : a;
    const uint64_t mask = __ballot(v != 0) & ~1ull;
    int len;
    lane_bits(lane, v, mask, 0, comp ? 1 : 0, len);
    if (lane == 0) len -= c_huff.dc[comp ? 1 : 0].ehuf[0] >> 16;   // the DC code is counted by the scan, from the difference
    len = wave_sum_int(len);
    if (live) {
        coef[g * 64 + lane] = (int16_t)v;
        if (lane == 0) blen[g] = len;
    }
}

// ---- 2. per image: full block bit counts -> bit offsets; zero the words blocks share
__global__ __launch_bounds__(1024) void jpeg_scan_kernel(const int16_t* __restrict__ coef, int* __restrict__ blen,
                                                         int64_t* __restrict__ boff, int64_t* __restrict__ tot_bits,
                                                         uint32_t* __restrict__ bits, int64_t img_words, int nblk) {
    __shared__ int64_t sh[1024];
    const int n = blockIdx.x, t = threadIdx.x;
    const int16_t* ci = coef + (int64_t)n * nblk * 64;
    int* li = blen + (int64_t)n * nblk;
    const int per = (nblk + 1023) / 1024, b0 = min(t * per, nblk), b1 = min(b0 + per, nblk);
    int64_t sum = 0;
    for (int b = b0; b < b1; ++b) {
        const int s = min(category(dc_diff(ci, b)), 11);
        const int l = li[b] + (int)(c_huff.dc[block_comp(b) ? 1 : 0].ehuf[s] >> 16) + s;
        li[b] = l;
        sum += l;
    }
    sh[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {   // inclusive Hillis-Steele scan
        const int64_t x = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    int64_t o = sh[t] - sum;
    uint32_t* wi = bits + (int64_t)n * img_words;
    for (int b = b0; b < b1; ++b) {
        boff[(int64_t)n * nblk + b] = o;
        wi[o >> 5] = 0;
        wi[(o + li[b] - 1) >> 5] = 0;
        o += li[b];
    }
    if (t == 1023) tot_bits[n] = sh[t];
}

// ---- 3. bit strings of every block into the image's bitstream (word bit 31 = first bit)
__global__ __launch_bounds__(64 * WAVES) void jpeg_emit_kernel(const int16_t* __restrict__ coef, const int* __restrict__ blen,
                                                               const int64_t* __restrict__ boff, uint32_t* __restrict__ bits,
                                                               int64_t img_words, int nblk, int64_t total) {
    constexpr int BUF = 128;   // >= (31 + 64 * 63 + 31) / 32 words
    __shared__ uint32_t buf[WAVES][BUF];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * WAVES + w;
    const bool live = g < total;
    const int64_t gg = live ? g : 0;
    const int n = (int)(gg / nblk), b = (int)(gg % nblk), comp = block_comp(b) ? 1 : 0;
    const int16_t* ci = coef + (int64_t)n * nblk * 64;
    const int v = ci[(int64_t)b * 64 + lane];
    const uint64_t mask = __ballot(v != 0) & ~1ull;
    int len;
    const uint64_t x = lane_bits(lane, v, mask, lane == 0 ? dc_diff(ci, b) : 0, comp, len);
    int pre = len;   // inclusive prefix sum over the wave
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(pre, o, 64);
        if (lane >= o) pre += y;
    }
    const int64_t base = boff[gg];
    const int o0 = (int)(base & 31);
    buf[w][lane] = 0;
    buf[w][lane + 64] = 0;
    __syncthreads();
    if (len) {
        const int p = o0 + pre - len, t = (p & 31) + len;   // t <= 31 + 63: the string spans <= 3 words
        const unsigned __int128 X = (unsigned __int128)x << (128 - t);
        uint32_t* dst = &buf[w][p >> 5];
        atomicOr(dst, (uint32_t)(X >> 96));
        if (t > 32) atomicOr(dst + 1, (uint32_t)(X >> 64));
        if (t > 64) atomicOr(dst + 2, (uint32_t)(X >> 32));
    }
    __syncthreads();
    if (!live) return;
    const int nwords = (o0 + blen[g] + 31) >> 5;
    uint32_t* out = bits + (int64_t)n * img_words + (base >> 5);
    for (int i = lane; i < nwords; i += 64) {
        const uint32_t val = buf[w][i];
        if (i == 0 || i == nwords - 1) {
            if (val) atomicOr(out + i, val);
        } else {
            out[i] = val;
        }
    }
}

__device__ inline int stream_byte(const uint32_t* wi, int64_t j, int64_t nbytes, int64_t L) {
    int v = (wi[j >> 2] >> (24 - 8 * (int)(j & 3))) & 0xff;
    if (j == nbytes - 1 && (L & 7)) v |= 0xff >> (L & 7);   // pad the final byte with 1-bits
    return v;
}

// ---- 4. 0xFF bytes per CHUNK of each image's entropy-coded segment
__global__ __launch_bounds__(256) void jpeg_ff_count_kernel(const uint32_t* __restrict__ bits, const int64_t* __restrict__ tot_bits,
                                                            int64_t img_words, int* __restrict__ chunk_ff, int nchunk) {
    __shared__ int sh[4];
    const int n = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
    const int64_t L = tot_bits[n], nbytes = (L + 7) >> 3;
    if ((int64_t)c * CHUNK >= nbytes) return;
    const uint32_t* wi = bits + (int64_t)n * img_words;
    const int64_t j0 = (int64_t)c * CHUNK + t * 16;
    int cnt = 0;
    for (int e = 0; e < 16; ++e)
        if (j0 + e < nbytes) cnt += stream_byte(wi, j0 + e, nbytes, L) == 0xff;
    cnt = wave_sum_int(cnt);
    if ((t & 63) == 0) sh[t >> 6] = cnt;
    __syncthreads();
    if (t == 0) chunk_ff[(int64_t)n * nchunk + c] = sh[0] + sh[1] + sh[2] + sh[3];
}

// ---- 5. per image: exclusive prefix of the chunk counts (in place), file size; header + EOI when files are written
__global__ __launch_bounds__(256) void jpeg_finish_kernel(int* __restrict__ chunk_ff, const int64_t* __restrict__ tot_bits, int nchunk,
                                                          int64_t* __restrict__ sizes, uint8_t* __restrict__ files, int64_t stride,
                                                          Header hdr) {
    __shared__ int64_t sh[256];
    const int n = blockIdx.x, t = threadIdx.x;
    const int64_t nbytes = (tot_bits[n] + 7) >> 3;
    const int used = (int)((nbytes + CHUNK - 1) / CHUNK);
    int* cf = chunk_ff + (int64_t)n * nchunk;
    const int per = (used + 255) / 256, c0 = min(t * per, used), c1 = min(c0 + per, used);
    int64_t sum = 0;
    for (int c = c0; c < c1; ++c) sum += cf[c];
    sh[t] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int64_t x = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    int64_t run = sh[t] - sum;
    for (int c = c0; c < c1; ++c) {
        const int k = cf[c];
        cf[c] = (int)run;
        run += k;
    }
    const int64_t size = HEADER_BYTES + nbytes + sh[255] + 2;
    if (t == 0) sizes[n] = size;
    if (files) {
        uint8_t* f = files + (int64_t)n * stride;
        for (int i = t; i < HEADER_BYTES; i += 256) f[i] = hdr.b[i];
        if (t == 0) { f[size - 2] = 0xff; f[size - 1] = 0xd9; }
    }
}

// ---- 6. entropy-coded bytes to their stuffed positions
__global__ __launch_bounds__(256) void jpeg_scatter_kernel(const uint32_t* __restrict__ bits, const int64_t* __restrict__ tot_bits,
                                                           int64_t img_words, const int* __restrict__ chunk_pre, int nchunk,
                                                           uint8_t* __restrict__ files, int64_t stride) {
    __shared__ int sh[256];
    const int n = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
    const int64_t L = tot_bits[n], nbytes = (L + 7) >> 3;
    if ((int64_t)c * CHUNK >= nbytes) return;
    const uint32_t* wi = bits + (int64_t)n * img_words;
    const int64_t j0 = (int64_t)c * CHUNK + t * 16;
    uint8_t by[16];
    int cnt = 0;
    for (int e = 0; e < 16; ++e) {
        by[e] = j0 + e < nbytes ? (uint8_t)stream_byte(wi, j0 + e, nbytes, L) : 0;
        cnt += j0 + e < nbytes && by[e] == 0xff;
    }
    sh[t] = cnt;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int x = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    int64_t pos = HEADER_BYTES + j0 + chunk_pre[(int64_t)n * nchunk + c] + sh[t] - cnt;
    uint8_t* f = files + (int64_t)n * stride;
    for (int e = 0; e < 16 && j0 + e < nbytes; ++e) {
        f[pos++] = by[e];
        if (by[e] == 0xff) f[pos++] = 0;
    }
}

// ---- host side
struct Geometry {
    int64_t nblk, img_words, nchunk;
    int64_t off_blen, off_boff, off_tot, off_chunk, off_bits, bytes;
};
static inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
static Geometry geometry(int N, int H, int W) {
    Geometry g;
    g.nblk = (int64_t)(H / 16) * (W / 16) * 6;
    const int64_t max_bytes = (g.nblk * MAX_BLOCK_BITS + 7) / 8;
    g.nchunk = (max_bytes + CHUNK - 1) / CHUNK;
    g.img_words = g.nchunk * (CHUNK / 4);
    g.off_blen = align256((int64_t)N * g.nblk * 64 * 2);
    g.off_boff = g.off_blen + align256((int64_t)N * g.nblk * 4);
    g.off_tot = g.off_boff + align256((int64_t)N * g.nblk * 8);
    g.off_chunk = g.off_tot + align256((int64_t)N * 8);
    g.off_bits = g.off_chunk + align256((int64_t)N * g.nchunk * 4);
    g.bytes = g.off_bits + (int64_t)N * g.img_words * 4;
    return g;
}
static bool geometry_ok(int H, int W) { return H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0 && H <= 65535 && W <= 65535; }

static void quant_tables(int quality, QuantTables& qt) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        const int l = (kLumaBase[k] * s + 50) / 100, c = (kChromaBase[k] * s + 50) / 100;
        qt.q[0][k] = (uint16_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
        qt.q[1][k] = (uint16_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
    }
}
// SOI, JFIF APP0 (v1.01, no density unit, 1:1, no thumbnail), DQT x2 (8-bit, zig-zag), SOF0, DHT x4, SOS -- 623 bytes
static void build_header(int H, int W, const QuantTables& qt, Header& h) {
    uint8_t* p = h.b;
    auto u8 = [&](int v) { *p++ = (uint8_t)v; };
    auto u16 = [&](int v) { u8(v >> 8); u8(v & 0xff); };
    u16(0xffd8);
    u16(0xffe0); u16(16); for (char ch : {'J', 'F', 'I', 'F', '\0'}) u8(ch);
    u8(1); u8(1); u8(0); u16(1); u16(1); u8(0); u8(0);
    for (int t = 0; t < 2; ++t) {
        u16(0xffdb); u16(67); u8(t);
        for (int k = 0; k < 64; ++k) u8(qt.q[t][kZigzagHost[k]]);
    }
    u16(0xffc0); u16(17); u8(8); u16(H); u16(W); u8(3);
    u8(1); u8(0x22); u8(0); u8(2); u8(0x11); u8(1); u8(3); u8(0x11); u8(1);
    auto dht = [&](int cls_id, const uint8_t (&nb)[16], const uint8_t* vals, int nv) {
        u16(0xffc4); u16(2 + 1 + 16 + nv); u8(cls_id);
        for (int i = 0; i < 16; ++i) u8(nb[i]);
        for (int i = 0; i < nv; ++i) u8(vals[i]);
    };
    dht(0x00, kDcLumaBits, kDcVals, 12);
    dht(0x10, kAcLumaBits, kAcLumaVals, 162);
    dht(0x01, kDcChromaBits, kDcVals, 12);
    dht(0x11, kAcChromaBits, kAcChromaVals, 162);
    u16(0xffda); u16(12); u8(3); u8(1); u8(0x00); u8(2); u8(0x11); u8(3); u8(0x11); u8(0); u8(63); u8(0);
}

}  // namespace jpg
}  // namespace advgrpo

using namespace advgrpo;

extern "C" int64_t advgrpo_jpeg_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || !jpg::geometry_ok(H, W)) return -1;
    return jpg::geometry(N, H, W).bytes;
}

extern "C" int64_t advgrpo_jpeg_max_file_bytes(int H, int W) {
    if (!jpg::geometry_ok(H, W)) return -1;
    const int64_t nblk = (int64_t)(H / 16) * (W / 16) * 6;
    // every entropy-coded byte may be a stuffed 0xFF: header + 2 * bytes + EOI
    return jpg::HEADER_BYTES + 2 * ((nblk * jpg::MAX_BLOCK_BITS + 7) / 8) + 2;
}

extern "C" int advgrpo_jpeg_encode(const void* images, int dtype, int layout, int N, int H, int W, int quality, int64_t* sizes,
                                   uint8_t* files, int64_t file_stride, void* workspace, int64_t workspace_bytes, void* stream) {
    ADVGRPO_CHECK(images && sizes && workspace, "jpeg_encode: null pointer (images, sizes and workspace are required)");
    ADVGRPO_CHECK(N > 0 && jpg::geometry_ok(H, W), "jpeg_encode: N, H, W must be positive and H, W multiples of 16 (<= 65535): got %d x %d x %d",
                  N, H, W);
    ADVGRPO_CHECK(quality >= 1 && quality <= 100, "jpeg_encode: quality %d outside 1..100", quality);
    ADVGRPO_CHECK(dtype == ADVGRPO_F32 || dtype == ADVGRPO_BF16 || dtype == ADVGRPO_U8, "jpeg_encode: unknown dtype %d", dtype);
    ADVGRPO_CHECK(layout == ADVGRPO_JPEG_NCHW || layout == ADVGRPO_JPEG_NHWC, "jpeg_encode: unknown layout %d", layout);
    const jpg::Geometry g = jpg::geometry(N, H, W);
    ADVGRPO_CHECK(workspace_bytes >= g.bytes, "jpeg_encode: workspace %lld bytes < %lld", (long long)workspace_bytes, (long long)g.bytes);
    ADVGRPO_CHECK(((uintptr_t)workspace & 255) == 0, "jpeg_encode: workspace must be 256-byte aligned");
    ADVGRPO_CHECK(!files || file_stride >= advgrpo_jpeg_max_file_bytes(H, W), "jpeg_encode: file_stride %lld < advgrpo_jpeg_max_file_bytes = %lld",
                  (long long)file_stride, (long long)advgrpo_jpeg_max_file_bytes(H, W));
    char* ws = (char*)workspace;
    int16_t* coef = (int16_t*)ws;
    int* blen = (int*)(ws + g.off_blen);
    int64_t* boff = (int64_t*)(ws + g.off_boff);
    int64_t* tot = (int64_t*)(ws + g.off_tot);
    int* chunk = (int*)(ws + g.off_chunk);
    uint32_t* bits = (uint32_t*)(ws + g.off_bits);
    jpg::QuantTables qt;
    jpg::quant_tables(quality, qt);
    hipStream_t s = as_stream(stream);
    const int64_t total = (int64_t)N * g.nblk;
    const int64_t grid = (total + jpg::WAVES - 1) / jpg::WAVES;
    ADVGRPO_CHECK(grid <= 0x7fffffff && g.nchunk <= 0x7fffffff && N <= 65535, "jpeg_encode: batch too large");
    hipLaunchKernelGGL(jpg::jpeg_dct_kernel, dim3((unsigned)grid), dim3(64 * jpg::WAVES), 0, s, images, dtype, layout, H, W, (int)g.nblk,
                       total, qt, coef, blen);
    hipLaunchKernelGGL(jpg::jpeg_scan_kernel, dim3(N), dim3(1024), 0, s, coef, blen, boff, tot, bits, g.img_words, (int)g.nblk);
    hipLaunchKernelGGL(jpg::jpeg_emit_kernel, dim3((unsigned)grid), dim3(64 * jpg::WAVES), 0, s, coef, blen, boff, bits, g.img_words,
                       (int)g.nblk, total);
    hipLaunchKernelGGL(jpg::jpeg_ff_count_kernel, dim3((unsigned)g.nchunk, N), dim3(256), 0, s, bits, tot, g.img_words, chunk, (int)g.nchunk);
    jpg::Header hdr{};
    if (files) jpg::build_header(H, W, qt, hdr);
    hipLaunchKernelGGL(jpg::jpeg_finish_kernel, dim3(N), dim3(256), 0, s, chunk, tot, (int)g.nchunk, sizes, files, file_stride, hdr);
    if (files)
        hipLaunchKernelGGL(jpg::jpeg_scatter_kernel, dim3((unsigned)g.nchunk, N), dim3(256), 0, s, bits, tot, g.img_words, chunk,
                           (int)g.nchunk, files, file_stride);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}
