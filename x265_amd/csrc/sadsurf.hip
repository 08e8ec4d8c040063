// sadsurf.hip — SAD surfaces behind x265hip_sadsurf_* (include/x265hip.h): the integer-pel candidates of the encoder's motion search as table loads.
//
// MotionEstimate::motionEstimate (reference source/encoder/motion.cpp:739-1569) measures an integer-pel candidate as
// sad(fenc, FENC_STRIDE, fref + mx + my * stride, stride) (:246-330) — a function of the source picture, the finished reference picture, the
// block's position and the vector, and of nothing the encoder decides.  One surface = one (source picture, reference picture) pair: for every
// aligned 16 / 32 / 64 block a 16 x 16 window of vectors, built by the kernels here as the reference picture's rows arrive and mirrored into page-locked
// host memory, where x265_amd/host/x265_hip_sadplanes.cpp reads them.  This file is the kernels and nothing else: the host side (surfbuild.hip) reaches
// them through the launch interface at the end (sadsurf.h), and the counter profiles stamped `# sources sadsurf.hip` cover exactly this text.
//
// The kernel is the search-window kernel of the design: one workgroup per 64 x 64 region (CTU), 16 waves.
//   stage    the source CTU (4 KB) and the reference window (64 + 2S)^2 around it (16 KB at S = 32) go to LDS once;
//   measure  wave b owns 16x16 block b of the CTU: its 256 source pixels sit in registers, and every vector of [-S, S)^2 is measured four at a
//            time with v_qsad_pk_u16_u8 (four SADs of 4 source pixels against a sliding 8-byte window of the reference row: 16 absolute
//            differences per lane and instruction, no alignment work), 64 instructions per four candidates; the 16 x (2S)^2 results
//            (u16, 128 KB at S = 32) stay in LDS — the exhaustive search's unique footprint per CTU is 4 KB + 16 KB in, nothing out;
//   decide   top down 64 -> 32 -> 16: a block's SAD at a vector is the sum of its 16x16 parts; cost = SAD + vector cost around the parent's
//            best vector; wave / workgroup minimum (DPP + LDS);
//   emit     the 16 x 16 window around each block's best vector is gathered out of the LDS surface (no second SAD pass) and written with the
//            block's origin into the CTU row's chunk of the table buffer.
// Values are pinned by tests/test_sadsurf.py (entries == sad<N, N> of the reference, pixel.cpp:40-55; origins == the same rule restated on the
// CPU by the test tier).  16-bit pictures (Main10 / Main12 builds) have a kernel of their own below: v_sad_u16, u32 surfaces — in LDS up to a range of 16, in
// device memory above it.
#include "common.h"
#include "sadsurf.h"
#include "surfplan.h"
#include "tiles.h"
#include <atomic>
#include <cstdlib>
#include <type_traits>

namespace xh {

// Which CTU of the launch a workgroup takes.  Workgroups are dealt to the eight XCDs round-robin in dispatch order (x fastest), and the windows of neighbouring
// CTUs overlap by half either way: in the plain order a row's neighbours sit in eight different L2s and each fetches the shared half again.  XCD x instead walks a
// contiguous run of CTUs: of the `total` workgroups it receives n_x = total / 8 + (x < total % 8) — the linear ids x, x + 8, ... — and its i-th takes CTU
// start_x + i, start_x = x * (total / 8) + min(x, total % 8): a bijection for any grid, every workgroup the same work.
__device__ __forceinline__ void surf_ctu(int xcd, int& cx, int& rowIn)
{
    cx = blockIdx.x; rowIn = blockIdx.y;
    if (!xcd) return;
    const int total = gridDim.x * gridDim.y, L = blockIdx.y * gridDim.x + blockIdx.x;
    const int x = L & 7, i = L >> 3, per = total >> 3, rem = total & 7;
    const int c = x * per + (x < rem ? x : rem) + i;
    cx = c % (int)gridDim.x; rowIn = c / (int)gridDim.x;
}

// ---- the kernel ---------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int ss_log(int d) { return 31 - __clz(4 * d + 1); }                  // floor(log2(4 d + 1)): bits(4 d) = 2 ss_log(d) + 1
__device__ __forceinline__ uint64_t u64_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
        const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
        v = u64_min(v, ((uint64_t)hi << 32) | lo);
    }
    return v;
}

// The scan of one block's candidates by a team of threads, four neighbouring vectors per step.  A thread owns the column group q (vectors
// vx = 4 q - S .. + 3) and the rows first, first + step, ...: its four horizontal terms are computed once.  `sums(c, s)` = the block's SADs at
// the candidates c .. c + 3.  cost = SAD + sVc[log(|vx - px|) + log(|vy - py|)] (the vector-cost table of this CTU's lambda), illegal vectors cost
// UINT_MAX; the thread's candidates are visited in ascending index, so `<` keeps the smallest index among equals.  Returns cost << 12 | index.
template <typename F>
__device__ __forceinline__ uint64_t ss_scan4(F sums, const uint32_t* sVc, int S, int q, int first, int step, int xlo, int xhi, int ylo, int yhi, int px, int py)
{
    const int D = 2 * S;
    uint32_t best = 0xFFFFFFFFu, bestC = 0;
    if (4 * q < D)
    {
        int lx[4];
        bool okx[4];
#pragma unroll
        for (int e = 0; e < 4; e++)
        {
            const int vx = 4 * q + e - S;
            lx[e] = ss_log(abs(vx - px));
            okx[e] = vx >= xlo && vx <= xhi;
        }
        for (int dyI = first; dyI < D; dyI += step)
        {
            const int vy = dyI - S;
            if (vy < ylo || vy > yhi)
                continue;
            const int ly = ss_log(abs(vy - py));
            const int c = dyI * D + 4 * q;
            uint32_t s[4];
            sums(c, s);
#pragma unroll
            for (int e = 0; e < 4; e++)
            {
                const uint32_t cost = okx[e] ? s[e] + sVc[lx[e] + ly] : 0xFFFFFFFFu;
                if (cost < best) { best = cost; bestC = (uint32_t)(c + e); }
            }
        }
    }
    return best == 0xFFFFFFFFu ? ~(uint64_t)0 : ((uint64_t)best << 12) | bestC;
}

__device__ __forceinline__ void ss_origin(uint64_t key, int S, int xlo, int xhi, int ylo, int yhi, int& bx, int& by, int& ox, int& oy)
{
    const int D = 2 * S;
    int c = (int)(key & 4095);
    if (key == ~(uint64_t)0) c = S * D + S;               // no legal candidate (cannot happen with margins >= S): vector (0, 0)
    by = c / D - S; bx = c - (c / D) * D - S;
    ox = bx - kWin / 2; oy = by - kWin / 2;
    if (ox > S - kWin) ox = S - kWin;
    if (ox < -S) ox = -S;
    if (oy > S - kWin) oy = S - kWin;
    if (oy < -S) oy = -S;
    if (ox > xhi - (kWin - 1)) ox = xhi - (kWin - 1);
    if (ox < xlo) ox = xlo;
    if (oy > yhi - (kWin - 1)) oy = yhi - (kWin - 1);
    if (oy < ylo) oy = ylo;
}

// four u16 SADs of one 16x16 block at the candidates c .. c + 3 (c a multiple of 4: one 8-byte LDS read), added to s[]
__device__ __forceinline__ void ss_add4(const uint16_t* surf, int c, uint32_t* s)
{
    const uint2 v = *(const uint2*)(surf + c);
    s[0] += v.x & 0xFFFFu; s[1] += v.x >> 16; s[2] += v.y & 0xFFFFu; s[3] += v.y >> 16;
}

// the same for the u32 surfaces of 16-bit pictures (one 16-byte LDS read)
__device__ __forceinline__ void ss_add4(const uint32_t* surf, int c, uint32_t* s)
{
    const uint4 v = *(const uint4*)(surf + c);
    s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
}

// what the phases of a workgroup share besides the surface
struct SsShared
{
    uint64_t red[16];
    int best[4][16][2];                                          // [level][block][vx, vy]
    int org[4][16][2];
    uint32_t vc[32];                                             // vector cost by log(|dx|) + log(|dy|)
};

// decide (top down 64 -> 32 -> 16) and emit the windows of levels 1..3 out of the LDS surface `sSurf` ([16][D][D], ST = u16 for 8-bit pictures, u32 for
// 16-bit ones); called by all 1024 threads of the workgroup after the surface is complete.  Leaves the level-1 origins in sh.org[1] (the 8x8 pass of
// the 8-bit kernel takes them from there).
template <typename ST>
__device__ __forceinline__ void ss_decide_emit(const SurfArgs& a, const SurfJob& jb, const ST* sSurf, SsShared& sh, int S, int x0, int y0, int cx, int cy)
{
    const int D = 2 * S, DD = D * D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t* sRed = sh.red;
    int (*sBest)[16][2] = sh.best;
    int (*sOrg)[16][2] = sh.org;
    const uint32_t* sVc = sh.vc;
    // ---- decide, top down ----
    // level 3: the whole CTU, all 1024 threads: column group tid & 15, rows tid >> 4, + 64, ...
    const bool have3 = x0 + 64 <= a.picW && y0 + 64 <= a.picH;
    if (have3)
    {
        const int xlo = -a.marginX - x0, xhi = a.picW + a.marginX - 64 - x0, ylo = -a.marginY - y0, yhi = a.picH + a.marginY - 64 - y0;
        uint64_t k = ss_scan4([&](int c, uint32_t* s) { s[0] = s[1] = s[2] = s[3] = 0;
#pragma unroll
                                                       for (int b = 0; b < 16; b++) ss_add4(sSurf + b * DD, c, s); },
                              sVc, S, tid & 15, tid >> 4, 64, xlo, xhi, ylo, yhi, 0, 0);
        k = wave_min_u64(k);
        if (lane == 0) sRed[wave] = k;
        __syncthreads();
        if (tid == 0)
        {
            uint64_t m = sRed[0];
            for (int i = 1; i < 16; i++) m = u64_min(m, sRed[i]);
            int bx, by, ox, oy;
            ss_origin(m, S, xlo, xhi, ylo, yhi, bx, by, ox, oy);
            sBest[3][0][0] = bx; sBest[3][0][1] = by; sOrg[3][0][0] = ox; sOrg[3][0][1] = oy;
        }
    }
    __syncthreads();
    // level 2: 32x32 block g <-> threads [256 g, 256 g + 256)
    {
        const int g = tid >> 8, t = tid & 255, gx = g & 1, gy = g >> 1;
        const int x = x0 + gx * 32, y = y0 + gy * 32;
        const bool have = x + 32 <= a.picW && y + 32 <= a.picH;
        const int xlo = -a.marginX - x, xhi = a.picW + a.marginX - 32 - x, ylo = -a.marginY - y, yhi = a.picH + a.marginY - 32 - y;
        uint64_t k = ~(uint64_t)0;
        if (have)
        {
            const int px = have3 ? sBest[3][0][0] : 0, py = have3 ? sBest[3][0][1] : 0;
            const ST* s0 = sSurf + ((gy * 2) * 4 + gx * 2) * DD;
            k = ss_scan4([&](int c, uint32_t* s) { s[0] = s[1] = s[2] = s[3] = 0;
                                                   ss_add4(s0, c, s); ss_add4(s0 + DD, c, s); ss_add4(s0 + 4 * DD, c, s); ss_add4(s0 + 5 * DD, c, s); },
                         sVc, S, t & 15, t >> 4, 16, xlo, xhi, ylo, yhi, px, py);
            k = wave_min_u64(k);
        }
        if (lane == 0) sRed[wave] = k;
        __syncthreads();
        if (have && t == 0)
        {
            uint64_t m = u64_min(u64_min(sRed[4 * g], sRed[4 * g + 1]), u64_min(sRed[4 * g + 2], sRed[4 * g + 3]));
            int bx, by, ox, oy;
            ss_origin(m, S, xlo, xhi, ylo, yhi, bx, by, ox, oy);
            sBest[2][g][0] = bx; sBest[2][g][1] = by; sOrg[2][g][0] = ox; sOrg[2][g][1] = oy;
        }
    }
    __syncthreads();
    // level 1: 16x16 block b <-> wave b
    {
        const int b = wave, bx16 = b & 3, by16 = b >> 2;
        const int x = x0 + bx16 * 16, y = y0 + by16 * 16;
        const bool have = x + 16 <= a.picW && y + 16 <= a.picH;
        if (have)
        {
            const int g = (by16 >> 1) * 2 + (bx16 >> 1);
            const bool haveParent = x0 + (bx16 >> 1) * 32 + 32 <= a.picW && y0 + (by16 >> 1) * 32 + 32 <= a.picH;
            const int px = haveParent ? sBest[2][g][0] : 0, py = haveParent ? sBest[2][g][1] : 0;
            const int xlo = -a.marginX - x, xhi = a.picW + a.marginX - 16 - x, ylo = -a.marginY - y, yhi = a.picH + a.marginY - 16 - y;
            const ST* s0 = sSurf + b * DD;
            uint64_t k = ss_scan4([&](int c, uint32_t* s) { s[0] = s[1] = s[2] = s[3] = 0; ss_add4(s0, c, s); },
                                  sVc, S, lane & 15, lane >> 4, 4, xlo, xhi, ylo, yhi, px, py);
            k = wave_min_u64(k);
            if (lane == 0)
            {
                int vx, vy, ox, oy;
                ss_origin(k, S, xlo, xhi, ylo, yhi, vx, vy, ox, oy);
                sOrg[1][b][0] = ox; sOrg[1][b][1] = oy;
            }
        }
    }
    __syncthreads();

    // ---- emit: origins and the 16 x 16 windows, gathered from the LDS surface ----
    char* chunk = jb.out + (int64_t)cy * a.pitch;
    // level 1: wave b, 4 entries per lane
    {
        const int b = wave, bx16 = b & 3, by16 = b >> 2;
        if (x0 + bx16 * 16 + 16 <= a.picW && y0 + by16 * 16 + 16 <= a.picH)
        {
            const int ox = sOrg[1][b][0], oy = sOrg[1][b][1];
            const int64_t idx = (int64_t)by16 * a.blocksX[1] + cx * 4 + bx16;
            if (lane == 0)
                *(uint32_t*)(chunk + a.originOff[1] + idx * 4) = (uint32_t)(uint16_t)(int16_t)ox | ((uint32_t)(uint16_t)(int16_t)oy << 16);
            const int j = lane >> 2, i4 = (lane & 3) * 4;
            const ST* p = sSurf + ((size_t)b * D + (oy + S + j)) * D + (ox + S + i4);
            const ST v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
            if (sizeof(ST) == 2)
            {
                uint16_t* tab = (uint16_t*)(chunk + a.tableOff[1]) + idx * (kWin * kWin);
                *(uint2*)(tab + j * kWin + i4) = make_uint2((uint32_t)v0 | ((uint32_t)v1 << 16), (uint32_t)v2 | ((uint32_t)v3 << 16));
            }
            else
            {
                uint32_t* tab = (uint32_t*)(chunk + a.tableOff[1]) + idx * (kWin * kWin);
                *(uint4*)(tab + j * kWin + i4) = make_uint4((uint32_t)v0, (uint32_t)v1, (uint32_t)v2, (uint32_t)v3);
            }
        }
    }
    // level 2: group g, one entry per thread
    {
        const int g = tid >> 8, t = tid & 255, gx = g & 1, gy = g >> 1;
        if (x0 + gx * 32 + 32 <= a.picW && y0 + gy * 32 + 32 <= a.picH)
        {
            const int ox = sOrg[2][g][0], oy = sOrg[2][g][1];
            const int64_t idx = (int64_t)gy * a.blocksX[2] + cx * 2 + gx;
            if (t == 0)
                *(uint32_t*)(chunk + a.originOff[2] + idx * 4) = (uint32_t)(uint16_t)(int16_t)ox | ((uint32_t)(uint16_t)(int16_t)oy << 16);
            const int j = t >> 4, i = t & 15, b0 = (gy * 2) * 4 + gx * 2;
            const size_t c = (size_t)(oy + S + j) * D + (ox + S + i);
            ((uint32_t*)(chunk + a.tableOff[2]))[idx * (kWin * kWin) + t] =
                (uint32_t)sSurf[b0 * DD + c] + sSurf[(b0 + 1) * DD + c] + sSurf[(b0 + 4) * DD + c] + sSurf[(b0 + 5) * DD + c];
        }
    }
    // level 3: threads 0..255
    if (have3 && tid < 256)
    {
        const int ox = sOrg[3][0][0], oy = sOrg[3][0][1];
        const int64_t idx = cx;
        if (tid == 0)
            *(uint32_t*)(chunk + a.originOff[3] + idx * 4) = (uint32_t)(uint16_t)(int16_t)ox | ((uint32_t)(uint16_t)(int16_t)oy << 16);
        const int j = tid >> 4, i = tid & 15;
        const size_t c = (size_t)(oy + S + j) * D + (ox + S + i);
        uint32_t t = 0;
#pragma unroll
        for (int b = 0; b < 16; b++) t += sSurf[b * DD + c];
        ((uint32_t*)(chunk + a.tableOff[3]))[idx * (kWin * kWin) + tid] = t;
    }

}

__global__ __launch_bounds__(1024) void sadsurf_ctu_kernel(SurfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ SsShared sh;

    int jn = 0, rowIn, cx;
    surf_ctu(a.xcd, cx, rowIn);
    while (jn + 1 < a.nJobs && rowIn >= a.job[jn].rows) { rowIn -= a.job[jn].rows; jn++; }
    const SurfJob& jb = a.job[jn];
    const int S = jb.S, D = 2 * S, DD = D * D;
    const int RW = 64 + D + 8;                                   // reference window row pitch (bytes): room for the last 24-byte read, multiple of 8
    uint8_t* sSrc = smem;                                        // [64][64]
    uint8_t* sRef = smem + 4096;                                 // [64 + D][RW]
    uint16_t* sSurf = (uint16_t*)(smem + 4096 + (size_t)(64 + D) * RW);      // [16][D][D]

    const int cy = jb.row0 + rowIn;
    const int x0 = cx * 64, y0 = cy * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.subpelOff3 >= 0 && cx < a.blocksX[3] && tid < X265HIP_SADSURF_SUBPEL)          // (blocksX: the blocks that lie inside the picture)
        ((uint32_t*)(jb.out + (int64_t)cy * a.pitch + a.subpelOff3))[(int64_t)cx * X265HIP_SADSURF_SUBPEL + tid] = 0;

    // ---- stage ----
    for (int i = tid; i < 64 * 16; i += 1024)
    {
        const int r = i >> 4, c4 = (i & 15) * 4;
        uint32_t v = 0;
        if (y0 + r < a.picH && x0 + c4 + 3 < a.picW)
            v = ld_global_unaligned<uint32_t>(jb.src + (int64_t)(y0 + r) * jb.srcPitch + x0 + c4);
        else if (y0 + r < a.picH)
            for (int k = 0; k < 4; k++)
                if (x0 + c4 + k < a.picW) v |= (uint32_t)jb.src[(int64_t)(y0 + r) * jb.srcPitch + x0 + c4 + k] << (8 * k);
        *(uint32_t*)(sSrc + r * 64 + c4) = v;
    }
    {
        const int dw = RW / 4;
        // the window may reach beyond the padded picture (small margins: CTU 16 pads 48 x 32; the last CTU row and column of any picture): those
        // positions belong to illegal vectors only — whatever is staged for them is never looked at — but the loads must stay inside the buffer
        const int yMax = a.bufRows - a.marginY - 1, xMax = a.picW + a.marginX - 4;
        for (int i = tid; i < (64 + D) * dw; i += 1024)
        {
            const int r = i / dw, c4 = (i - r * dw) * 4;
            const int y = min(max(y0 - S + r, -a.marginY), yMax), x = min(max(x0 - S + c4, -a.marginX), xMax);
            *(uint32_t*)(sRef + r * RW + c4) = ld_global_unaligned<uint32_t>(jb.ref + (int64_t)y * jb.refStride + x);
        }
    }
    if (tid < 32)
        sh.vc[tid] = (uint32_t)((jb.lambda20 * (2 * tid + 2) + 10) / 20);        // bits(4 |dx|) + bits(4 |dy|) = 2 (log + log) + 2
    __syncthreads();

    // ---- measure: wave b <-> 16x16 block b.  A lane owns an 8 x 8 patch of vectors: 16 accumulators of four u16 SADs each.  Reference row j of
    // the patch (24 bytes) is read once and meets source row j - dy for each of the patch's eight dy: 64 v_qsad_pk_u16_u8 per 24 bytes of LDS ----
    {
        const int b = wave, bx = b & 3, by = b >> 2;
        const bool inside = x0 + bx * 16 + 16 <= a.picW && y0 + by * 16 + 16 <= a.picH;
        if (inside)
        {
            uint32_t s[16][4];
#pragma unroll
            for (int r = 0; r < 16; r++)
            {
                // the block's pixels are the same for every lane of the wave: scalar registers, the qsad's second operand
                const uint4 v = *(const uint4*)(sSrc + (by * 16 + r) * 64 + bx * 16);
                s[r][0] = __builtin_amdgcn_readfirstlane(v.x); s[r][1] = __builtin_amdgcn_readfirstlane(v.y);
                s[r][2] = __builtin_amdgcn_readfirstlane(v.z); s[r][3] = __builtin_amdgcn_readfirstlane(v.w);
            }
            const int G = D / 8;
            for (int item = lane; item < G * G; item += 64)
            {
                const int dyg = item / G, xs = item - dyg * G;
                const uint8_t* base = sRef + (by * 16 + 8 * dyg) * RW + bx * 16 + 8 * xs;
                uint64_t acc[8][2];
#pragma unroll
                for (int i = 0; i < 8; i++) acc[i][0] = acc[i][1] = 0;
#pragma unroll
                for (int j = 0; j < 23; j++)
                {
                    const uint2* p = (const uint2*)(base + j * RW);
                    const uint2 p0 = p[0], p1 = p[1], p2 = p[2];
                    const uint32_t d[6] = { p0.x, p0.y, p1.x, p1.y, p2.x, p2.y };
#pragma unroll
                    for (int dyo = 0; dyo < 8; dyo++)
                    {
                        const int r = j - dyo;
                        if (r < 0 || r > 15)
                            continue;
#pragma unroll
                        for (int k = 0; k < 4; k++)
                        {
                            acc[dyo][0] = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)d[k + 1] << 32) | d[k], s[r][k], acc[dyo][0]);
                            acc[dyo][1] = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)d[k + 2] << 32) | d[k + 1], s[r][k], acc[dyo][1]);
                        }
                    }
                }
                // an accumulator's u16 lanes hold at most 16 * 16 * 255 = 65280: no carry between them
                uint16_t* o = sSurf + ((size_t)b * D + 8 * dyg) * D + 8 * xs;
#pragma unroll
                for (int dyo = 0; dyo < 8; dyo++)
                    *(uint4*)(o + dyo * D) = make_uint4((uint32_t)acc[dyo][0], (uint32_t)(acc[dyo][0] >> 32), (uint32_t)acc[dyo][1], (uint32_t)(acc[dyo][1] >> 32));
            }
        }
    }
    __syncthreads();

    ss_decide_emit<uint16_t>(a, jb, sSurf, sh, S, x0, y0, cx, cy);
    char* chunk = jb.out + (int64_t)cy * a.pitch;
    const auto& sOrg = sh.org;
    // level 0: the four 8x8 blocks of wave b's 16x16 block take their parent's window; their SADs are measured now, 4 vectors per lane (one row of
    // the window = 4 lanes): per source row two v_qsad_pk_u16_u8 on a 12-byte stretch of the reference row, brought to byte alignment with
    // v_alignbyte (the window's origin is arbitrary).  An 8x8 block whose parent is not inside the picture has no window: origin (-32768, -32768)
    {
        const int b = wave, bx16 = b & 3, by16 = b >> 2;
        const bool parent = x0 + bx16 * 16 + 16 <= a.picW && y0 + by16 * 16 + 16 <= a.picH;
        const int ox = parent ? sOrg[1][b][0] : 0, oy = parent ? sOrg[1][b][1] : 0;
#pragma unroll 1
        for (int q = 0; q < (jb.level0 ? 4 : 0); q++)
        {
            const int qx = q & 1, qy = q >> 1;
            const int x = x0 + bx16 * 16 + qx * 8, y = y0 + by16 * 16 + qy * 8;
            if (x + 8 > a.picW || y + 8 > a.picH)
                continue;
            const int64_t idx = (int64_t)(by16 * 2 + qy) * a.blocksX[0] + cx * 8 + bx16 * 2 + qx;
            if (!parent)
            {
                if (lane == 0)
                    *(uint32_t*)(chunk + a.originOff[0] + idx * 4) = 0x80008000u;
                *(uint2*)((uint16_t*)(chunk + a.tableOff[0]) + idx * (kWin * kWin) + lane * 4) = make_uint2(0, 0);
                continue;
            }
            if (lane == 0)
                *(uint32_t*)(chunk + a.originOff[0] + idx * 4) = (uint32_t)(uint16_t)(int16_t)ox | ((uint32_t)(uint16_t)(int16_t)oy << 16);
            const int j = lane >> 2, i4 = (lane & 3) * 4;
            const int col = bx16 * 16 + qx * 8 + ox + S + i4, sh = col & 3;
            const uint8_t* rp0 = sRef + (by16 * 16 + qy * 8 + oy + S + j) * RW + (col - sh);
            const uint8_t* sp0 = sSrc + (by16 * 16 + qy * 8) * 64 + bx16 * 16 + qx * 8;
            uint64_t acc = 0;
#pragma unroll
            for (int r = 0; r < 8; r++)
            {
                const uint2 sv = *(const uint2*)(sp0 + r * 64);
                const uint32_t s0 = __builtin_amdgcn_readfirstlane(sv.x), s1 = __builtin_amdgcn_readfirstlane(sv.y);
                const uint32_t* w = (const uint32_t*)(rp0 + r * RW);
                const uint32_t d0 = w[0], d1 = w[1], d2 = w[2], d3 = w[3];
                const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, sh), w1 = __builtin_amdgcn_alignbyte(d2, d1, sh), w2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)w1 << 32) | w0, s0, acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)w2 << 32) | w1, s1, acc);
            }
            uint16_t* tab = (uint16_t*)(chunk + a.tableOff[0]) + idx * (kWin * kWin);
            *(uint2*)(tab + j * kWin + i4) = make_uint2((uint32_t)acc, (uint32_t)(acc >> 32));
        }
    }
}

// ---- the same kernel for 16-bit pictures (Main10 / Main12 builds) --------------------------------------------------------------------------
// v_qsad_pk_u16_u8 is a byte instruction; 16-bit samples are measured with v_sad_u16 (two absolute differences per lane and instruction), and a 16x16
// SAD no longer fits 16 bits, so the surface holds u32 — 16 x (2 S)^2 x 4 bytes: S <= 16 keeps it in LDS (64 KB), see ss16_ctu for larger S.  The reference window is staged twice,
// once as it is and once shifted by one sample, so that odd vectors read aligned dwords too.  A lane owns a 4 x 4 patch of vectors; the block's source
// rows go through scalar registers eight at a time.  Decide and emit are the shared template.
//
// Ranges above 16 (S = 20 .. 32): 16 x (2 S)^2 x 4 bytes is up to 256 KB, more than a CU's LDS, so the surface of such a CTU lies in device memory — Wide: `surfaces`
// is the workgroup's own region of a pooled buffer.  Stage and measure are the same code (the patch's sixteen results leave as four 16-byte global stores instead
// of four LDS stores); decide and emit read the region through the same template (a workgroup lives on one CU: its stores are visible to its other waves behind the
// barrier's workgroup-scope fence).  LDS then holds the source CTU and the two windows only: 76 KB at S = 32.  Measured: 3.4 x the S = 16 launch for 4 x the
// vectors (profiles/r09_v1_sadsurf16_range.txt), which is why the surface is not cut into strips that fit LDS instead.
template <bool Wide>
__device__ __forceinline__ void ss16_ctu(const SurfArgs& a, unsigned char* smem, SsShared& sh, uint32_t* surfaces, int cx, int rowIn)
{
    int jn = 0;
    while (jn + 1 < a.nJobs && rowIn >= a.job[jn].rows) { rowIn -= a.job[jn].rows; jn++; }
    const SurfJob& jb = a.job[jn];
    const int S = jb.S, D = 2 * S;
    const int RWD = (64 + D) / 2 + 4;                            // window row pitch in dwords (two samples each): room for the last 9-dword read, even
    uint32_t* sSrc = (uint32_t*)smem;                            // [64][32] dwords
    uint32_t* sRefA = sSrc + 64 * 32;                            // [64 + D][RWD]: dword k = samples (2k, 2k + 1) of the window row
    uint32_t* sRefB = sRefA + (64 + D) * RWD;                    // the same shifted by one sample: dword k = samples (2k + 1, 2k + 2)
    uint32_t* sSurf = Wide ? surfaces : sRefB + (64 + D) * RWD;  // [16][D][D]

    const int cy = jb.row0 + rowIn;
    const int x0 = cx * 64, y0 = cy * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.subpelOff3 >= 0 && cx < a.blocksX[3] && tid < X265HIP_SADSURF_SUBPEL)          // (as in the 8-bit kernel: 10-bit pictures' tables are summed over quadrant jobs too)
        ((uint32_t*)(jb.out + (int64_t)cy * a.pitch + a.subpelOff3))[(int64_t)cx * X265HIP_SADSURF_SUBPEL + tid] = 0;
    const uint16_t* src = (const uint16_t*)jb.src;
    const uint16_t* ref = (const uint16_t*)jb.ref;
    const int64_t srcPitch = jb.srcPitch / 2;                    // samples

    // ---- stage ----
    for (int i = tid; i < 64 * 32; i += 1024)
    {
        const int r = i >> 5, c2 = (i & 31) * 2;
        uint32_t v = 0;
        if (y0 + r < a.picH)
        {
            if (x0 + c2 < a.picW) v = src[(int64_t)(y0 + r) * srcPitch + x0 + c2];
            if (x0 + c2 + 1 < a.picW) v |= (uint32_t)src[(int64_t)(y0 + r) * srcPitch + x0 + c2 + 1] << 16;
        }
        sSrc[r * 32 + c2 / 2] = v;
    }
    {
        // positions outside the padded picture's buffer belong to illegal vectors only: the loads are clamped into the buffer (see the 8-bit kernel)
        // (sample pairs start at even positions and the padded width is even: a pair is inside or outside as a whole; the third sample is clamped alone)
        const int yMax = a.bufRows - a.marginY - 1, xEnd = a.picW + a.marginX;
        for (int i = tid; i < (64 + D) * RWD; i += 1024)
        {
            const int r = i / RWD, k = i - r * RWD;
            const int y = min(max(y0 - S + r, -a.marginY), yMax), x = min(max(x0 - S + 2 * k, -a.marginX), xEnd - 2);
            const uint16_t* p = ref + (int64_t)y * jb.refStride;
            const uint32_t s0 = p[x], s1 = p[x + 1], s2 = p[min(x + 2, xEnd - 1)];
            sRefA[r * RWD + k] = s0 | (s1 << 16);
            sRefB[r * RWD + k] = s1 | (s2 << 16);
        }
    }
    if (tid < 32)
        sh.vc[tid] = (uint32_t)((jb.lambda20 * (2 * tid + 2) + 10) / 20);
    __syncthreads();

    // ---- measure: wave b <-> 16x16 block b; a lane owns 4 x 4 vectors (16 u32 accumulators); source rows eight at a time in scalar registers ----
    {
        const int b = wave, bx = b & 3, by = b >> 2;
        const bool inside = x0 + bx * 16 + 16 <= a.picW && y0 + by * 16 + 16 <= a.picH;
        if (inside)
        {
            const int G = D / 4;
            for (int item = lane; item < G * G; item += 64)
            {
                const int py4 = item / G, px4 = item - py4 * G;
                uint32_t acc[4][4];
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int c = 0; c < 4; c++) acc[i][c] = 0;
#pragma unroll 1
                for (int h = 0; h < 2; h++)
                {
                    uint32_t s[8][8];
#pragma unroll
                    for (int r = 0; r < 8; r++)
                    {
                        const uint4 v0 = *(const uint4*)(sSrc + (by * 16 + 8 * h + r) * 32 + bx * 8), v1 = *(const uint4*)(sSrc + (by * 16 + 8 * h + r) * 32 + bx * 8 + 4);
                        s[r][0] = __builtin_amdgcn_readfirstlane(v0.x); s[r][1] = __builtin_amdgcn_readfirstlane(v0.y);
                        s[r][2] = __builtin_amdgcn_readfirstlane(v0.z); s[r][3] = __builtin_amdgcn_readfirstlane(v0.w);
                        s[r][4] = __builtin_amdgcn_readfirstlane(v1.x); s[r][5] = __builtin_amdgcn_readfirstlane(v1.y);
                        s[r][6] = __builtin_amdgcn_readfirstlane(v1.z); s[r][7] = __builtin_amdgcn_readfirstlane(v1.w);
                    }
                    const int base = (by * 16 + 8 * h + 4 * py4) * RWD + bx * 8 + 2 * px4;
#pragma unroll
                    for (int j = 0; j < 11; j++)
                    {
                        const uint32_t* pa = sRefA + base + j * RWD;
                        const uint32_t* pb = sRefB + base + j * RWD;
                        uint32_t da[9], db[9];
#pragma unroll
                        for (int k = 0; k < 4; k++)
                        {
                            const uint2 va = *(const uint2*)(pa + 2 * k), vb = *(const uint2*)(pb + 2 * k);
                            da[2 * k] = va.x; da[2 * k + 1] = va.y; db[2 * k] = vb.x; db[2 * k + 1] = vb.y;
                        }
                        da[8] = pa[8]; db[8] = pb[8];
#pragma unroll
                        for (int dyo = 0; dyo < 4; dyo++)
                        {
                            const int r = j - dyo;
                            if (r < 0 || r > 7)
                                continue;
#pragma unroll
                            for (int k = 0; k < 8; k++)
                            {
                                acc[dyo][0] = __builtin_amdgcn_sad_u16(da[k], s[r][k], acc[dyo][0]);
                                acc[dyo][1] = __builtin_amdgcn_sad_u16(db[k], s[r][k], acc[dyo][1]);
                                acc[dyo][2] = __builtin_amdgcn_sad_u16(da[k + 1], s[r][k], acc[dyo][2]);
                                acc[dyo][3] = __builtin_amdgcn_sad_u16(db[k + 1], s[r][k], acc[dyo][3]);
                            }
                        }
                    }
                }
                uint32_t* o = sSurf + ((size_t)b * D + 4 * py4) * D + 4 * px4;
#pragma unroll
                for (int dyo = 0; dyo < 4; dyo++)
                    *(uint4*)(o + dyo * D) = make_uint4(acc[dyo][0], acc[dyo][1], acc[dyo][2], acc[dyo][3]);
            }
        }
    }
    __syncthreads();

    ss_decide_emit<uint32_t>(a, jb, sSurf, sh, S, x0, y0, cx, cy);
}

__global__ __launch_bounds__(1024) void sadsurf_ctu16_kernel(SurfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ SsShared sh;

    int rowIn, cx;
    surf_ctu(a.xcd, cx, rowIn);
    ss16_ctu<false>(a, smem, sh, nullptr, cx, rowIn);
}

// The wide form's launch: a bounded 1-D grid (the pooled buffer holds one region of `regionElems` u32 per workgroup, so the grid is what the device can hold at
// once, not the CTU count); workgroup g takes the CTUs g, g + grid, ... of the launch's `total` = cols x rows, in surf_ctu's XCD order restated for linear ids
// (workgroup L of a round goes to XCD L % 8 when the grid is a multiple of 8; any grid gives a bijection).
__global__ __launch_bounds__(1024) void sadsurf_ctu16_wide_kernel(SurfArgs a, uint32_t* surfaces, int64_t regionElems, int cols, int total)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ SsShared sh;

    uint32_t* mine = surfaces + (int64_t)blockIdx.x * regionElems;
    for (int L = blockIdx.x; L < total; L += gridDim.x)
    {
        int c = L;
        if (a.xcd)
        {
            const int x = L & 7, i = L >> 3, per = total >> 3, rem = total & 7;
            c = x * per + (x < rem ? x : rem) + i;
        }
        ss16_ctu<true>(a, smem, sh, mine, c % cols, c / cols);
        __syncthreads();                                         // the next CTU's staging and measure overwrite what this one's emit reads
    }
}


// ---- sub-pel SATD tables (round 4) ---------------------------------------------------------------------------------------------------------------
// What MotionEstimate::subpelCompare (reference encoder/motion.cpp:1571-1600) computes with the satd comparison — satd(source block, reference block
// at quarter-pel vector q), the reference block being the picture itself (q integer) or luma_hpp / vpp / hvpp of it, i.e. the mirror's phase plane
// 4 fy + fx — for the 7 x 7 vectors q = 4 c + (dx, dy) around the window's centre c = origin + WIN / 2 of every block of levels 1..3.  A job = one
// (block, vector); a wave runs 64 / T jobs at once, T = lanes per job (one 4x4 tile each per step), as pixcmp_kernel<SATD> does (pixel.hip); the SATD of
// a 16x16 / 32x32 / 64x64 block is the sum over its 4x4 tiles of (sum |H d H^T|) >> 1 (pixel.cpp:210-297: satd8<w, h> over satd_8x4).
template <typename P>
__global__ __launch_bounds__(256) void subpel_satd_kernel(SubpelArgs a)
{
    const int lane = threadIdx.x & 63;
    // XCD-aware order: workgroups are dealt to the eight XCDs round-robin, each XCD has its own L2, and consecutive jobs — the 49 vectors of a block, then the next
    // block of the row, whose phase-plane lines are the same 128-byte lines — want ONE L2.  The job order is cut into chunks of 16 workgroups, chunk c goes to
    // XCD c % 8: workgroup b (XCD b % 8, its i-th there, i = b / 8) takes place ((i / 16) * 8 + b % 8) * 16 + i % 16.  Chunks rather than one contiguous eighth
    // per XCD: the levels have few jobs each (64x64 blocks: 368 workgroups' worth per picture row set) and an eighth-per-XCD split leaves XCDs without work —
    // measured 95.9 us per launch against 77.2 us in the plain order, with the HBM fetch already down 5.3 x.  The grid is a multiple of 128.
    // X265HIP_SADSURF_XCD=0 (a.xcd == 0): the plain order
    const int xi = (int)(blockIdx.x >> 3), xq = (int)(blockIdx.x & 7);
    const int vblock = a.xcd ? (((xi >> 4) * 8 + xq) << 4) + (xi & 15) : (int)blockIdx.x;
    const int gwave = vblock * (blockDim.x >> 6) + (threadIdx.x >> 6), wavesTotal = gridDim.x * (blockDim.x >> 6);
    const P* pic = (const P*)a.pic;
    const P* planes = (const P*)a.planes;
    for (int l = 1; l < 4; l++)
    {
        const int N = 8 << l, tiles = (N >> 2) * (N >> 2), T = tiles >= 64 ? 64 : tiles, bpw = 64 / T, iters = tiles / T;
        const int n = a.jobs[l] - a.jobs[l - 1], sub = lane & (T - 1);
        const int rowBlocks = a.per[l] * a.blocksX[l];
        for (int job0 = gwave * bpw; job0 < n; job0 += wavesTotal * bpw)
        {
            const int job = job0 + lane / T;
            int jc = job < n ? job : n - 1;
            int v = jc % X265HIP_SADSURF_SUBPEL, b = jc / X265HIP_SADSURF_SUBPEL;           // b: block index inside the launch's rows of this level
            int cr = a.row0 + b / rowBlocks, k = b % rowBlocks;                             // chunk (row of 64 lines), index inside the chunk
            int by = cr * a.per[l] + k / a.blocksX[l];
            // block rows below the picture (a last CTU row that is not 64 lines tall) exist in the chunk's layout but not in the pictures: such lanes
            // (and the lanes past the last job) measure the picture's first block instead (its origin was written by this launch or an earlier one) and
            // store nothing
            const bool ok = job < n && by < a.blocksY[l];
            if (!ok) { v = 0; cr = 0; k = 0; by = 0; }
            const int bx = k % a.blocksX[l];
            const bool inPic = ok;
            char* chunk = a.out + (int64_t)cr * a.pitch;
            const int16_t* org = (const int16_t*)(chunk + a.originOff[l]) + 2 * k;
            const int cx = org[0] + kWin / 2, cy = org[1] + kWin / 2;
            const int qx = 4 * cx + v % 7 - 3, qy = 4 * cy + v / 7 - 3;
            const int phase = 4 * (qy & 3) + (qx & 3);
            const P* ref = (phase ? planes + (int64_t)phase * a.planeElems : pic) + (int64_t)(by * N + (qy >> 2)) * a.stride + bx * N + (qx >> 2);
            const P* srcB = (const P*)((const char*)a.src + (int64_t)(by * N) * a.srcPitch) + bx * N;
            const int64_t srcStride = a.srcPitch / (int64_t)sizeof(P);
            int acc = 0;
            for (int it = 0; it < iters; it++)
            {
                const int t = sub + it * T, ty = (t / (N >> 2)) * 4, tx = (t % (N >> 2)) * 4;
                int m[16];
                tile_diff(srcB + ty * srcStride + tx, srcStride, ref + ty * a.stride + tx, a.stride, m);
                hadamard4x4(m);
                acc += abs_sum16(m) >> 1;
            }
            acc = group_sum(acc, T);
            if (ok && inPic && sub == 0)
                ((uint32_t*)(chunk + a.subpelOff[l]))[(int64_t)k * X265HIP_SADSURF_SUBPEL + v] = (uint32_t)acc;
        }
    }
}

// ---- the same tables for 8-bit pictures, second form (round 6): the planes through LDS, the lanes are the vectors, packed 16-bit Hadamard --------------------
// subpel_satd_kernel above measures a (block, vector) per group of lanes, a lane per 4x4 tile: eight scattered 4-byte global loads and ~160 VALU instructions per
// tile and vector — the texture addresser and the VALU are both near their limits (ISA count; the planes' lines come out of L2).  Here a workgroup takes a
// block: the block's footprint in the sixteen phase planes — (Q + 1) rows of Q + 1 pixels around the window's centre, whole dwords — is staged in LDS ONCE for
// the 49 vectors, lane v measures vector v and walks the block's tiles: a tile's four rows are four ds_read2_b32 (the two dwords a row of four unaligned pixels
// lies in) and two v_perm_b32 each with the lane's own byte selectors, which split them into 16-bit pairs at the same time.  The Hadamard runs on packed pairs
// (|coefficients| <= 16 * 255; common.h), and it is LINEAR: the source tile's transform M s is made once per tile (64 lanes, one tile each, into LDS) and
// a lane accumulates sum |M s - M r| with v_sad_u16 — two coefficients and the accumulation per instruction.  v_sad_u16 compares unsigned halves: both
// transforms carry the same bias 0x4000 in their first sample, which reaches every coefficient as +-0x4000 and cancels in the difference.  M is the Hadamard up
// to the sign of every other coefficient (the rotate-and-multiply butterfly below), the same for both sides.  ~57 VALU instructions per tile and vector
// instead of ~160, no scattered global loads.  A tile's sum of magnitudes is even (it is congruent to the sum of the coefficients = 16 x the first sample), so
// shifting the block's total once equals pixel.cpp:210-297's shift per 8x4.
// Jobs of a launch, all of one size (one staging, 16 tiles per wave): the four 32x32 quadrants of every 64x64 block (their halved sums meet in the entry by
// atomicAdd; the window kernel zeroes those entries), the 32x32 blocks (the four waves take 16 tiles each), the 16x16 blocks four to a workgroup (a block per
// wave).  X265HIP_SUBPEL_LDS=0: the first form.
namespace sp8 {
// geometry of a staged block, in dwords: B bytes per pixel, Q x Q block -> Q + 1 rows of Q + 1 pixels starting at any pixel: whole dwords, Q B / 4 + 1 per row
template <int B, int Q> struct Lay { static constexpr int pitch = Q * B / 4 + 1, plane = (Q + 1) * pitch, block = 16 * plane; };
template <int B> constexpr int ref_dw() { return (4 * Lay<B, 16>::block > Lay<B, 32>::block ? 4 * Lay<B, 16>::block : Lay<B, 32>::block) + 4; }
struct Geo { int ok, x0, y0, sx, sy, k, cr, pad; };      // footprint's first pixel (x0, y0) in the reference, the block's (quadrant's) first pixel (sx, sy) in the source
}

// rows as ((c0, c1), (c2, c3)) pairs in, M * tile out (see above)
__device__ __forceinline__ void pk_hadamard4x4(s2v a[4], s2v b[4])
{
    const s2v kh = { 1, -1 };
#pragma unroll
    for (int h = 0; h < 2; h++)
    {
        s2v* v = h ? b : a;
        const s2v s0 = v[0] + v[1], e0 = v[0] - v[1], s1 = v[2] + v[3], e1 = v[2] - v[3];
        v[0] = s0 + s1; v[1] = e0 + e1; v[2] = s0 - s1; v[3] = e0 - e1;
    }
#pragma unroll
    for (int y = 0; y < 4; y++)
    {
        const s2v A = a[y] + b[y], B = a[y] - b[y];
        const s2v Ar = as_s2(__builtin_amdgcn_alignbit(as_u(A), as_u(A), 16)), Br = as_s2(__builtin_amdgcn_alignbit(as_u(B), as_u(B), 16));
        a[y] = Ar * kh + A; b[y] = Br * kh + B;
    }
}

// stage ONE block's footprint (Q x Q block, B bytes per pixel) with a group of T threads (a wave or the workgroup), g = the thread's number in the group; (x0, y0) is
// uniform over the group, so a load is a scalar base + a 32-bit offset.  Every thread issues ALL its loads before the first LDS store (a load -> wait -> store loop
// has one 4-byte load in flight per thread: twenty round trips to L2 per staging).  The picture (plane 0) has an allocation of its own; planes 1..15 follow one another.
template <int B, int Q, int T>
__device__ __forceinline__ void sp8_stage_ref(const SubpelArgs& a, int x0, int y0, int g, uint32_t* dst)
{
    constexpr int pitch = sp8::Lay<B, Q>::pitch, planeDw = sp8::Lay<B, Q>::plane, n15 = 15 * planeDw, it0 = (planeDw + T - 1) / T, it15 = (n15 + T - 1) / T;
    const int64_t first = ((int64_t)y0 * a.stride + x0) * B;
    // buffer loads: the 128-bit descriptor of a group-uniform base in scalar registers + ONE 32-bit offset register per load (a flat address is two, and the
    // compiler builds all of a batch's addresses before its first load: 157 registers with global_load, three waves per SIMD)
    const __amdgpu_buffer_rsrc_t d0 = __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)a.pic + (uintptr_t)first) & ~(uintptr_t)3), 0, (int)0xfffffff0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t d1 = __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)a.planes + (uintptr_t)(a.planeElems * B) + (uintptr_t)first) & ~(uintptr_t)3), 0, (int)0xfffffff0u, 0x00020000);
    const uint32_t stride = (uint32_t)a.stride * B, planeBytes = (uint32_t)a.planeElems * B;
    uint32_t v0[it0], v1[it15];
#pragma unroll
    for (int k = 0; k < it0; k++)
    {
        const int i0 = g + T * k, i = i0 < planeDw ? i0 : planeDw - 1, r = i / pitch, j = i - r * pitch;
        v0[k] = __builtin_amdgcn_raw_buffer_load_b32(d0, (int)((uint32_t)r * stride + 4u * (uint32_t)j), 0, 0);
    }
#pragma unroll
    for (int k = 0; k < it15; k++)
    {
        const int i0 = g + T * k, i = i0 < n15 ? i0 : n15 - 1, pp = i / planeDw, r1 = i - pp * planeDw, r = r1 / pitch, j = r1 - r * pitch;
        v1[k] = __builtin_amdgcn_raw_buffer_load_b32(d1, (int)((uint32_t)pp * planeBytes + (uint32_t)r * stride + 4u * (uint32_t)j), 0, 0);
    }
#pragma unroll
    for (int k = 0; k < it0; k++)
        if (g + T * k < planeDw) dst[g + T * k] = v0[k];
#pragma unroll
    for (int k = 0; k < it15; k++)
        if (g + T * k < n15) dst[planeDw + g + T * k] = v1[k];
}
// the transform of one source tile per thread: tile t of the Q x Q block whose first pixel is (sx, sy)
template <typename P, int Q>
__device__ __forceinline__ void sp8_stage_src(const SubpelArgs& a, int sx, int sy, int t, uint32_t* o)
{
    typedef typename std::conditional<sizeof(P) == 1, uint32_t, uint2>::type Row;
    constexpr int TX = Q / 4;
    const int ty = t / TX, tx = t - ty * TX;
    const P* s = (const P*)((const char*)a.src + (int64_t)(sy + 4 * ty) * a.srcPitch) + sx + 4 * tx;
    const int64_t srcStride = a.srcPitch / (int64_t)sizeof(P);
    s2v sa[4], sb[4];
#pragma unroll
    for (int y = 0; y < 4; y++)
        Pk16<P>::split(ld_global_unaligned<Row>(s + y * srcStride), sa[y], sb[y]);
    sa[0] = as_s2(as_u(sa[0]) | 0x4000u);
    pk_hadamard4x4(sa, sb);
    *(uint4*)o = make_uint4(as_u(sa[0]), as_u(sa[1]), as_u(sa[2]), as_u(sa[3]));
    *(uint4*)(o + 4) = make_uint4(as_u(sb[0]), as_u(sb[1]), as_u(sb[2]), as_u(sb[3]));
}

// sum over tiles [t0, t1) of a staged block of sum |M s - M r| for this lane's vector: `ref` = the lane's first dword in the staged footprint.  8 bit: a row of
// four pixels lies in two dwords, (selLo, selHi) pick its bytes into 16-bit pairs.  16 bit: in three, the pairs are dwords (d0, d1) or — an odd first pixel —
// the middles of (d0, d1) and (d1, d2): ONE selector (selLo) for both v_perm_b32
template <int B, int Q>
__device__ __forceinline__ uint32_t sp8_tiles(const uint32_t* ref, uint32_t selLo, uint32_t selHi, const uint32_t* hs, int t0, int t1)
{
    constexpr int pitch = sp8::Lay<B, Q>::pitch, TX = Q / 4;
    uint32_t acc = 0;
#pragma unroll 2
    for (int t = t0; t < t1; t++)
    {
        const int ty = t / TX, tx = t - ty * TX;
        const uint32_t* p = ref + 4 * ty * pitch + tx * B;
        s2v ra[4], rb[4];
#pragma unroll
        for (int y = 0; y < 4; y++)
        {
            const uint32_t d0 = p[y * pitch], d1 = p[y * pitch + 1];
            if (B == 1)
            {
                ra[y] = as_s2(__builtin_amdgcn_perm(d1, d0, selLo));
                rb[y] = as_s2(__builtin_amdgcn_perm(d1, d0, selHi));
            }
            else
            {
                const uint32_t d2 = p[y * pitch + 2];
                ra[y] = as_s2(__builtin_amdgcn_perm(d1, d0, selLo));
                rb[y] = as_s2(__builtin_amdgcn_perm(d2, d1, selLo));
            }
        }
        ra[0] = as_s2(as_u(ra[0]) | 0x4000u);
        pk_hadamard4x4(ra, rb);
        const uint4 h0 = *(const uint4*)(hs + 8 * t), h1 = *(const uint4*)(hs + 8 * t + 4);
        acc = __builtin_amdgcn_sad_u16(as_u(ra[0]), h0.x, acc); acc = __builtin_amdgcn_sad_u16(as_u(ra[1]), h0.y, acc);
        acc = __builtin_amdgcn_sad_u16(as_u(ra[2]), h0.z, acc); acc = __builtin_amdgcn_sad_u16(as_u(ra[3]), h0.w, acc);
        acc = __builtin_amdgcn_sad_u16(as_u(rb[0]), h1.x, acc); acc = __builtin_amdgcn_sad_u16(as_u(rb[1]), h1.y, acc);
        acc = __builtin_amdgcn_sad_u16(as_u(rb[2]), h1.z, acc); acc = __builtin_amdgcn_sad_u16(as_u(rb[3]), h1.w, acc);
    }
    return acc;
}

// P = uint8_t: 8-bit pictures; uint16_t: 10-bit pictures (|coefficients| <= 16 * 1023 = 16 368: inside 16 bits with the bias; 12-bit pictures keep the first form)
template <typename P>
__global__ __launch_bounds__(256) void subpel_satd_kernel_lds(SubpelArgs a)
{
    constexpr int B = (int)sizeof(P);
    typedef sp8::Lay<B, 16> L16;
    typedef sp8::Lay<B, 32> L32;
    __shared__ uint32_t sRef[sp8::ref_dw<B>()];
    __shared__ __attribute__((aligned(16))) uint32_t sHs[64 * 8];
    __shared__ uint32_t sPart[4 * 64];
    __shared__ sp8::Geo sGeo[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = (a.jobs[1] - a.jobs[0]) / X265HIP_SADSURF_SUBPEL, n2 = (a.jobs[2] - a.jobs[1]) / X265HIP_SADSURF_SUBPEL, n3 = (a.jobs[3] - a.jobs[2]) / X265HIP_SADSURF_SUBPEL;
    const int total = 4 * n3 + n2 + ((n1 + 3) >> 2);
    // the lane's vector: quarter-pel offset (dx, dy) from the centre -> phase plane 4 fy + fx at the whole-pel offset (dx >> 2, dy >> 2) = -1 or 0
    const int v = lane < X265HIP_SADSURF_SUBPEL ? lane : 0;
    const int dx = v % 7 - 3, dy = v / 7 - 3, phase = 4 * (dy & 3) + (dx & 3);
    const int xi = (int)(blockIdx.x >> 3), xq = (int)(blockIdx.x & 7);
    const int first = a.xcd ? (((xi >> 4) * 8 + xq) << 4) + (xi & 15) : (int)blockIdx.x;          // (subpel_satd_kernel: chunks of 16 workgroups per XCD)
    for (int job = first; job < total; job += gridDim.x)
    {
        // a 64x64 block is four jobs, one per 32x32 quadrant: every job is ONE staging + 16 tiles per wave (a workgroup that walked the four quadrants itself was
        // the launch's long pole: a launch is ~180 CTUs, two rounds of workgroups).  A quadrant's sum is even like a tile's, so the halves add up to the block's
        // entry: atomicAdd into entries the window kernel of the same rows has zeroed (SurfArgs::subpelOff3)
        const int l = job < 4 * n3 ? 3 : job < 4 * n3 + n2 ? 2 : 1;
        const int b0 = l == 3 ? job >> 2 : l == 2 ? job - 4 * n3 : 4 * (job - 4 * n3 - n2), quad = l == 3 ? job & 3 : 0;
        const int nb = l == 1 ? (n1 - b0 < 4 ? n1 - b0 : 4) : 1, N = 8 << l;
        const int rowBlocks = a.per[l] * a.blocksX[l];
        __syncthreads();                                                             // the previous job's LDS is no longer read
        if (tid < 4)
        {
            sp8::Geo g = { 0, 0, 0, 0, 0, 0, 0, 0 };
            if (tid < nb)
            {
                const int b = b0 + tid;
                g.cr = a.row0 + b / rowBlocks; g.k = b % rowBlocks;
                const int by = g.cr * a.per[l] + g.k / a.blocksX[l], bx = g.k % a.blocksX[l];
                g.ok = by < a.blocksY[l];
                if (g.ok)
                {
                    const int16_t* org = (const int16_t*)(a.out + (int64_t)g.cr * a.pitch + a.originOff[l]) + 2 * g.k;
                    g.sx = bx * N + 32 * (quad & 1); g.sy = by * N + 32 * (quad >> 1);
                    g.x0 = g.sx + org[0] + kWin / 2 - 1; g.y0 = g.sy + org[1] + kWin / 2 - 1;
                }
            }
            sGeo[tid] = g;
        }
        __syncthreads();
        {
            // (blocks that do not exist carry the geometry of the picture's first block: valid addresses, nothing of them is kept)
            const sp8::Geo& gs = sGeo[l == 1 ? wave : 0];
            const int x0 = __builtin_amdgcn_readfirstlane(gs.x0), y0 = __builtin_amdgcn_readfirstlane(gs.y0);
            if (l == 1) sp8_stage_ref<B, 16, 64>(a, x0, y0, lane, sRef + wave * L16::block);
            else sp8_stage_ref<B, 32, 256>(a, x0, y0, tid, sRef);
            if (tid < 64)
            {
                const sp8::Geo& gt = sGeo[l == 1 ? tid >> 4 : 0];
                if (gt.ok)
                {
                    if (l == 1) sp8_stage_src<P, 16>(a, gt.sx, gt.sy, tid & 15, sHs + 8 * tid);
                    else sp8_stage_src<P, 32>(a, gt.sx, gt.sy, tid, sHs + 8 * tid);
                }
            }
        }
        __syncthreads();
        const sp8::Geo& g = sGeo[l == 1 ? wave : 0];
        uint32_t acc = 0;
        if (g.ok)
        {
            // alignment of the footprint's first pixel in its dword: the planes share one (planeElems and the stride are multiples of 4 bytes), the picture has its own
            // allocation.  col = the lane's first pixel in the staged row, counted in pixels from the row's first dword
            const uintptr_t base = phase ? (uintptr_t)a.planes : (uintptr_t)a.pic;
            const int col = (int)(((base + (uintptr_t)(((int64_t)g.y0 * a.stride + g.x0) * B)) & 3) / B) + 1 + (dx >> 2);
            constexpr int perDw = 4 / B;
            const int sh = col & (perDw - 1), dw = col / perDw;
            const uint32_t selLo = B == 1 ? ((uint32_t)sh | 0x0c000c00u | ((uint32_t)(sh + 1) << 16)) : (sh ? 0x05040302u : 0x03020100u);
            const uint32_t selHi = (uint32_t)(sh + 2) | 0x0c000c00u | ((uint32_t)(sh + 3) << 16);
            if (l == 1)
                acc = sp8_tiles<B, 16>(sRef + wave * L16::block + phase * L16::plane + (1 + (dy >> 2)) * L16::pitch + dw, selLo, selHi, sHs + wave * 16 * 8, 0, 16);
            else
                acc = sp8_tiles<B, 32>(sRef + phase * L32::plane + (1 + (dy >> 2)) * L32::pitch + dw, selLo, selHi, sHs, 16 * wave, 16 * wave + 16);
        }
        if (l == 1)
        {
            if (g.ok && lane < X265HIP_SADSURF_SUBPEL)
                ((uint32_t*)(a.out + (int64_t)g.cr * a.pitch + a.subpelOff[l]))[(int64_t)g.k * X265HIP_SADSURF_SUBPEL + lane] = acc >> 1;
        }
        else
        {
            sPart[tid] = acc;
            __syncthreads();
            if (g.ok && tid < X265HIP_SADSURF_SUBPEL)
            {
                uint32_t* o = (uint32_t*)(a.out + (int64_t)g.cr * a.pitch + a.subpelOff[l]) + (int64_t)g.k * X265HIP_SADSURF_SUBPEL + tid;
                const uint32_t sum = (sPart[tid] + sPart[64 + tid] + sPart[128 + tid] + sPart[192 + tid]) >> 1;
                if (l == 3) atomicAdd(o, sum);
                else *o = sum;
            }
        }
    }
}


// ---- the launch interface (sadsurf.h): the only way the builder reaches the kernels above ----------------------------------------------------

static size_t surf_lds_bytes(int S)
{
    const int D = 2 * S, RW = 64 + D + 8;
    return 4096 + (size_t)(64 + D) * RW + (size_t)16 * D * D * 2;
}

static size_t surf16_lds_bytes(int S)
{
    const int D = 2 * S, RWD = (64 + D) / 2 + 4;
    return (size_t)64 * 32 * 4 + (size_t)2 * (64 + D) * RWD * 4 + (size_t)16 * D * D * 4;
}

// the wide form (16-bit pictures, S > 16): the source CTU and the two windows; the surface is a region of a pooled device buffer
static size_t surf16_wide_lds_bytes(int S)
{
    const int D = 2 * S, RWD = (64 + D) / 2 + 4;
    return (size_t)64 * 32 * 4 + (size_t)2 * (64 + D) * RWD * 4;
}
bool surf16_wide(int depth, int S) { return depth != 8 && S > 16; }

// the dynamic LDS limit is a per-device attribute of the kernel
bool raise_lds_limits(int dev)
{
    static std::atomic<uint64_t> attrSet{ 0 };
    if (!(attrSet.load() >> dev & 1))
    {
        if (hipFuncSetAttribute((const void*)sadsurf_ctu_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)surf_lds_bytes(32)) != hipSuccess ||
            hipFuncSetAttribute((const void*)sadsurf_ctu16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)surf16_lds_bytes(16)) != hipSuccess ||
            hipFuncSetAttribute((const void*)sadsurf_ctu16_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)surf16_wide_lds_bytes(32)) != hipSuccess)
            return false;
        attrSet |= (uint64_t)1 << dev;
    }
    return true;
}

bool launch_windows(const SurfArgs& a, int depth, int maxS, int cols, int rows, hipStream_t st, char* wideBuf, int wideGroups)
{
    if (depth == 8)
        hipLaunchKernelGGL(sadsurf_ctu_kernel, dim3(cols, rows), dim3(1024), surf_lds_bytes(maxS), st, a);
    else if (surf16_wide(depth, maxS))
        hipLaunchKernelGGL(sadsurf_ctu16_wide_kernel, dim3(wideGroups), dim3(1024), surf16_wide_lds_bytes(maxS), st, a, (uint32_t*)wideBuf, (int64_t)16 * (2 * maxS) * (2 * maxS), cols,
                           cols * rows);
    else
        hipLaunchKernelGGL(sadsurf_ctu16_kernel, dim3(cols, rows), dim3(1024), surf16_lds_bytes(maxS), st, a);
    return hipGetLastError() == hipSuccess;
}

bool launch_subpel(const SubpelArgs& sa, int depth, int B, bool quadrantSums, hipStream_t st)
{
    static const bool ldsForm = !(getenv("X265HIP_SUBPEL_LDS") && !atoi(getenv("X265HIP_SUBPEL_LDS")));
    // the second form adds the quadrants of a 64x64 block into its entries: only behind a window kernel that has zeroed them (subpel_quadrant_sums); it
    // stages whole dwords, so the reference's rows and planes must start on one
    if (quadrantSums && (depth == 8 || depth == 10) && ldsForm && sa.stride * B % 4 == 0 && sa.planeElems * B % 4 == 0)
    {
        const int blocks1 = sa.jobs[1] / X265HIP_SADSURF_SUBPEL, blocks2 = (sa.jobs[2] - sa.jobs[1]) / X265HIP_SADSURF_SUBPEL, blocks3 = (sa.jobs[3] - sa.jobs[2]) / X265HIP_SADSURF_SUBPEL;
        const int grid = plan::subpel_lds_grid(plan::subpel_lds_groups(blocks1, blocks2, blocks3));
        if (depth == 8)
            hipLaunchKernelGGL(subpel_satd_kernel_lds<uint8_t>, dim3(grid), dim3(256), 0, st, sa);
        else
            hipLaunchKernelGGL(subpel_satd_kernel_lds<uint16_t>, dim3(grid), dim3(256), 0, st, sa);
    }
    else if (depth == 8)
        hipLaunchKernelGGL(subpel_satd_kernel<uint8_t>, dim3(plan::subpel_grid(plan::subpel_waves(sa.jobs))), dim3(256), 0, st, sa);
    else
        hipLaunchKernelGGL(subpel_satd_kernel<uint16_t>, dim3(plan::subpel_grid(plan::subpel_waves(sa.jobs))), dim3(256), 0, st, sa);
    return hipGetLastError() == hipSuccess;
}

} // namespace xh
