// Prototype gate for the matrix-core key switch: k_keyswitch_mfma against the shipped k_keyswitch_waves on
// the same box in the same process, at a full default shape, from a synthetic key image and uniform random operand words.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/ubench_ks_mfma.hip -o tools/_ubench_ks_mfma
//   tools/_ubench_ks_mfma [n = 500] [reps = 200] [S ...]        (default S list: the sweep 64 ... 2048)
// For every S: both kernels run once from the same (0, ..., 0, b) rows and every output word is compared (integers: they
// must be equal, not close); then each is timed over `reps` back-to-back launches, old / new / old / new, and the better
// of the two passes is printed.  Exit status 1 on any mismatch.
#include "../eoc_tfhe_amd/csrc/kernels.hip.h"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
using namespace eoc;

#define CK(x)                                                                        \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(2);                                                                 \
        }                                                                            \
    } while (0)

__global__ void k_fill(uint32_t *p, size_t nwords, uint64_t seed)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull + seed; // splitmix64
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        p[i] = (uint32_t)((x ^ (x >> 31)) >> 16);
    }
}
__global__ void k_rows(int32_t *out, uint32_t S, int n)
{ // (0, ..., 0, b): what k_ks_init leaves
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)S * (n + 1); i += (size_t)gridDim.x * blockDim.x)
        out[i] = (int)(i % (n + 1)) == n ? (int32_t)(0x1234567u * (uint32_t)(i / (n + 1))) : 0;
}

template <int NWV, int IW>
static void run_old(const KSArgs &a, uint32_t S, int ncb)
{
    typedef KS3Cfg<8, NWV, IW> C;
    static bool attr = false;
    if (!attr) {
        CK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_keyswitch_waves<8, NWV, IW>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
        attr = true;
    }
    const uint32_t ntiles = (S + 63) / 64;
    hipLaunchKernelGGL((k_keyswitch_waves<8, NWV, IW>), dim3(ntiles * ncb * C::NS, 1), dim3(64 * NWV), C::LDS_BYTES, 0,
                       (const GateDesc *)nullptr, a);
}
static void launch_old(const KSArgs &a, uint32_t S)
{
    const int ncb = a.n1p / 64;
    if (ncb == 4) run_old<8, 16>(a, S, ncb);
    else if (ncb == 8) run_old<8, 32>(a, S, ncb);
    else if (ncb == 12) run_old<4, 64>(a, S, ncb);
    else run_old<8, 64>(a, S, ncb);
}
static KSMPlan plan_of(uint32_t S, int n1p)
{ // KS_NWV = 4 | 8 and KS_NSL = 1 ... 64 (a power of two) override the library's plan: the sweep behind ks_mfma_plan
    KSMPlan pl = ks_mfma_plan(S, n1p);
    if (getenv("KS_NWV")) pl.nwv = atoi(getenv("KS_NWV")) == 8 ? 8 : 4;
    if (getenv("KS_NSL")) pl.nsl = atoi(getenv("KS_NSL"));
    if (pl.nsl < 1 || pl.nsl > 64 || (pl.nsl & (pl.nsl - 1))) exit(2);
    pl.gx = (S + 64 * pl.nwv - 1) / (64 * pl.nwv) * (unsigned)(n1p / 32) * (unsigned)pl.nsl;
    return pl;
}
static void launch_new(const KSArgs &a, uint32_t S, const int8_t *limbs)
{
    const KSMPlan pl = plan_of(S, a.n1p);
    if (pl.nwv == 8) // the alternative the library's plan never picks and the library no longer compiles: instantiated here
        hipLaunchKernelGGL(k_keyswitch_mfma<8>, dim3(pl.gx, 1), dim3(512), 0, 0, nullptr, a, reinterpret_cast<const i4 *>(limbs), pl.nsl);
    else
        ks_mfma_launch(pl, 1, nullptr, a, limbs, 0);
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 500;
    const int reps = argc > 2 ? atoi(argv[2]) : 200;
    std::vector<uint32_t> Ss;
    for (int k = 3; k < argc; k++) Ss.push_back((uint32_t)atoi(argv[k]));
    if (Ss.empty()) Ss = {64, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048};
    uint32_t Smax = 0;
    for (uint32_t s : Ss) Smax = s > Smax ? s : Smax;
    const int n1p = (n + 1 + 255) / 256 * 256;
    const size_t ksk_words = (size_t)kN * 8 * 3 * n1p, limb_bytes = ks_limb_bytes(n1p);

    int32_t *d_ksk, *d_o1, *d_o2;
    uint32_t *d_ubar;
    int8_t *d_limbs;
    CK(hipMalloc(&d_ksk, ksk_words * 4));
    CK(hipMalloc(&d_limbs, limb_bytes));
    CK(hipMalloc(&d_ubar, (size_t)Smax * kN * 4));
    CK(hipMalloc(&d_o1, (size_t)Smax * (n + 1) * 4));
    CK(hipMalloc(&d_o2, (size_t)Smax * (n + 1) * 4));
    k_fill<<<4096, 256>>>((uint32_t *)d_ksk, ksk_words, 1);
    // the image's padding columns are zero in the engine; here they are random on purpose (col > n must be masked)
    k_fill<<<4096, 256>>>(d_ubar, (size_t)Smax * kN, 2);
    ks_limbs_launch(d_ksk, d_limbs, n1p, 0);
    CK(hipDeviceSynchronize());
    printf("n %d n1p %d: key image %.1f MB, limb image %.1f MB\n", n, n1p, ksk_words * 4 / 1e6, limb_bytes / 1e6);

    KSArgs a;
    a.ksk = d_ksk;
    a.u = nullptr;
    a.ubar = d_ubar;
    a.n = n;
    a.n1p = n1p;
    a.t = 8;
    a.basebit = 2;
    a.mu = 0;
    a.inline_desc = 1;
    a.desc0 = GateDesc{0, 0, nullptr, nullptr, nullptr, nullptr};

    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    int bad_total = 0;
    std::vector<int32_t> h1, h2;
    for (uint32_t S : Ss) {
        a.S = S;
        const size_t ow = (size_t)S * (n + 1);
        k_rows<<<1024, 256>>>(d_o1, S, n);
        k_rows<<<1024, 256>>>(d_o2, S, n);
        a.desc0.out = d_o1;
        launch_old(a, S);
        a.desc0.out = d_o2;
        launch_new(a, S, d_limbs);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        h1.resize(ow);
        h2.resize(ow);
        CK(hipMemcpy(h1.data(), d_o1, ow * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(h2.data(), d_o2, ow * 4, hipMemcpyDeviceToHost));
        size_t bad = 0, nz = 0;
        for (size_t k = 0; k < ow; k++) {
            bad += h1[k] != h2[k];
            nz += h1[k] != 0;
        }
        if (bad) {
            bad_total++;
            for (size_t k = 0, shown = 0; k < ow && shown < 8; k++)
                if (h1[k] != h2[k]) {
                    printf("  row %zu col %zu: old %08x new %08x\n", k / (n + 1), k % (n + 1), h1[k], h2[k]);
                    shown++;
                }
        }
        float best[2] = {1e9f, 1e9f};
        for (int pass = 0; pass < 2; pass++)
            for (int which = 0; which < 2; which++) {
                a.desc0.out = which ? d_o2 : d_o1;
                for (int r = 0; r < 10; r++) which ? launch_new(a, S, d_limbs) : launch_old(a, S);
                CK(hipEventRecord(e0, 0));
                for (int r = 0; r < reps; r++) which ? launch_new(a, S, d_limbs) : launch_old(a, S);
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                float ms;
                CK(hipEventElapsedTime(&ms, e0, e1));
                ms /= reps;
                best[which] = ms < best[which] ? ms : best[which];
            }
        const KSMPlan pl = plan_of(S, n1p);
        printf("S %5u: words differing %zu of %zu (nonzero %zu)  waves %.4f ms  mfma %.4f ms  ratio %.3f  [waves/wg %d slices %d]\n",
               S, bad, ow, nz, best[0], best[1], best[1] / best[0], pl.nwv, pl.nsl);
        fflush(stdout);
    }
    return bad_total ? 1 : 0;
}
