/*
 * eoc_tfhe_gpu.h -- C ABI of libeoc_tfhe_gpu.so, the MI355X-native gate-bootstrapping engine that
 * sits behind the eoc-tfhe Lua/C surface.
 *
 * Conventions are the reference's (ao-tfhe/eoc-tfhe-run.h:8-19, ao-tfhe/eoc-tfhe-run.cpp:167-513):
 *   - plain C symbols, plain pointers and sizes, no exceptions across the boundary
 *     (the reference is built -fno-exceptions, ao-tfhe/build.sh:23);
 *   - string functions return a heap C string the caller releases with free() (the binding does
 *     exactly that, ao-tfhe/eoc-tfhe-bindings.c:21,35,47,65,75,86,112) or NULL on error with a
 *     message on stderr (eoc-tfhe-run.cpp:218-219,277-278); int functions return a negative code;
 *   - one process-global key context for the string API (globalSecretKey / globalPublicKey,
 *     eoc-tfhe-run.cpp:38-40); every base64Key / public_key argument is accepted and ignored,
 *     as the bindings pass NULL (ao-tfhe/eoc-tfhe-bindings.c:63,73,84,97,110).
 *
 * Three layers, lowest first:
 *   1. engine API  (eoc_engine_*, eoc_*_device): device pointers + a HIP stream; what bench.py and
 *      a multi-GPU host use.  This is where libtfhe's bootsNAND/.../bootsMUX -> tfhe_bootstrap_FFT
 *      -> tfhe_blindRotate_FFT -> lweKeySwitch would be bound (upstream tfhe/tfhe@bc71bfae, absent
 *      from /root/reference; call-stack in SURVEY.md 3.3).
 *   2. batch API   (eoc_keygen, eoc_encrypt_bits, eoc_gate_batch, eoc_circuit_run): caller-owned
 *      host buffers of int32 LWE samples.
 *   3. string API  (encryptBit, gateNAND, ...): base64 in / base64 out, the exact style of
 *      addCiphertexts (eoc-tfhe-run.cpp:427-470) so that `l_gate*` wrappers follow
 *      l_addCiphertexts (ao-tfhe/eoc-tfhe-bindings.c:12-24) line for line.
 *
 * The gate path has NO CPU fallback: without a usable HIP device every hot-path entry point
 * fails (negative code / NULL and a message on stderr).
 */
#ifndef EOC_TFHE_GPU_H
#define EOC_TFHE_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOC_N 1024 /* ring degree, fixed (k = 1) */

/* TFheGateBootstrappingParameterSet (type used at eoc-tfhe-run.cpp:230) flattened. */
typedef struct eoc_params {
    int32_t n;          /* LWE dimension, 1 ... 1023 */
    int32_t l;          /* gadget length, 1 ... 4 */
    int32_t Bgbit;      /* log2 gadget base; l * Bgbit <= 32 and, for an engine, l * 2^Bgbit <= 8192: beyond that an
                           external-product coefficient (bounded by l * Bg * 2^41) outgrows what the FP64 transform and its
                           conversion are specified for (see eoc_dbg_fft_inv_device) and eoc_engine_create refuses the shape */
    int32_t ks_t;       /* key-switch length */
    int32_t ks_basebit; /* log2 key-switch base */
    double ks_stdev;    /* LWE / fresh-ciphertext / key-switch-key noise */
    double bk_stdev;    /* bootstrapping-key noise */
} eoc_params;

/* gate opcodes: libtfhe's boots* family (SURVEY.md 8a a1,a2) */
enum eoc_op {
    EOC_NAND = 0, EOC_AND = 1, EOC_OR = 2, EOC_NOR = 3, EOC_XOR = 4, EOC_XNOR = 5,
    EOC_ANDNY = 6, EOC_ANDYN = 7, EOC_ORNY = 8, EOC_ORYN = 9, EOC_MUX = 10,
    EOC_NOT = 11, EOC_COPY = 12,
    EOC_CONST0 = 13, EOC_CONST1 = 14, /* bootsCONSTANT(result, 0 / 1): noiseless trivial sample, no inputs (in0 = -1 / NULL) */
    /* EXTENSION gates (round 6) -- not in libtfhe's boots* family, built from its primitives the way bootsXOR is: a linear
     * stage over THREE samples (lweAddTo / lweAddMulTo, no constant), then tfhe_bootstrap_FFT with mu = 1/8.
     *   EOC_MAJ (a, b, c)  t = a + b + c: the phases are +-1/8 or +-3/8 and the sign is the MAJORITY -- a full adder's carry
     *                      (and, with a negated input, a subtractor's borrow / a comparator's step) in ONE bootstrap
     *   EOC_XOR3(a, b, c)  t = -2 (a + b + c): the phases are +-1/4 and the sign is the PARITY -- a full adder's sum
     * One blind rotation and one key switch each, like the two-input gates; same decision margins (1/8 and 1/4). */
    EOC_MAJ = 15, EOC_XOR3 = 16
};

/* error codes (all negative) */
enum {
    EOC_OK = 0, EOC_ERR_ARG = -1, EOC_ERR_NO_DEVICE = -2, EOC_ERR_HIP = -3, EOC_ERR_NO_KEY = -4,
    EOC_ERR_ALLOC = -5, EOC_ERR_STATE = -6
};

/* replaces new_default_gate_bootstrapping_parameters(minimum_lambda) (eoc-tfhe-run.cpp:230).
 * set 0 = "A" (n=500, l=2, Bgbit=10; BASELINE.json's numbers), set 1 = "B" (n=630, l=3, Bgbit=7;
 * what minimum_lambda=128 selects at the pinned libtfhe).  eoc_params_for_lambda mirrors the
 * lambda switch: lambda <= 80 -> A, 81..128 -> B, else error. */
int eoc_default_params(int set, eoc_params *out);
int eoc_params_for_lambda(int minimum_lambda, eoc_params *out);

/* ------------------------------------------------------------------------------------------------
 * client side (CPU): keys, encryption, decryption
 * replaces new_random_gate_bootstrapping_secret_keyset (eoc-tfhe-run.cpp:231), bootsSymEncrypt /
 * bootsSymDecrypt (upstream), lweSymEncrypt / lwePhase (eoc-tfhe-run.cpp:149,161,291,411)
 * ---------------------------------------------------------------------------------------------- */
typedef struct eoc_secret_key eoc_secret_key; /* TFheGateBootstrappingSecretKeySet */

/* Randomness.  Two modes:
 *   eoc_keygen(seed)    REPRODUCIBLE / TEST mode (PRNG v1): counter streams of the splitmix64 finaliser keyed by the
 *                       64-bit seed, the generator the oracle shares, so keys and ciphertexts compare bit for bit.
 *                       NOT secure: the finaliser is invertible and the seed is short; public masks reveal the
 *                       stream key.  The same holds for eoc_encrypt_bits / eoc_lwe_encrypt with an explicit enc_seed.
 *   eoc_keygen_secure   PRNG v2: a 256-bit master key from getrandom(2); every stream is ChaCha20 under its own
 *                       sub-key.  eoc_encrypt_bits_keyed is the matching encryption under a caller-held 256-bit key.
 * The string / global API (generateGateKey with seed 0, generateSecretKey, encryptBit, eoc_global_encrypt_bits, ...)
 * uses the secure mode with encryption randomness drawn fresh per process, independent of the key material. */
int eoc_keygen(const eoc_params *p, uint64_t seed, int with_cloud_key, eoc_secret_key **out);
int eoc_keygen_secure(const eoc_params *p, int with_cloud_key, eoc_secret_key **out);
int eoc_keygen_from_master(const eoc_params *p, const uint8_t master[32], int with_cloud_key, eoc_secret_key **out);
int eoc_sk_is_secure(const eoc_secret_key *sk);
int eoc_encrypt_bits_keyed(const eoc_secret_key *sk, const uint8_t enc_key[32], uint64_t first_idx,
                           const uint8_t *bits, size_t count, int32_t *cts);
/* RFC 8439 block function (known-answer test of the generator behind the secure mode) */
void eoc_dbg_chacha20_block(const uint8_t key[32], uint32_t counter, const uint8_t nonce[12], uint8_t out[64]);
void eoc_secret_key_free(eoc_secret_key *sk);
const eoc_params *eoc_sk_params(const eoc_secret_key *sk);
const int32_t *eoc_sk_lwe_key(const eoc_secret_key *sk);  /* [n]   bits */
const int32_t *eoc_sk_tlwe_key(const eoc_secret_key *sk); /* [N]   bits */
const int32_t *eoc_sk_bk(const eoc_secret_key *sk);       /* [n][2l][2][N] torus32, or NULL */
const int32_t *eoc_sk_ksk(const eoc_secret_key *sk);      /* [N*t*(base-1)][n+1], or NULL */
size_t eoc_bk_len(const eoc_params *p);                   /* int32 count of the two arrays above */
size_t eoc_ksk_len(const eoc_params *p);

/* bits[count] -> cts[count][n+1]; sample s uses stream (enc_seed, first_idx + s) */
int eoc_encrypt_bits(const eoc_secret_key *sk, uint64_t enc_seed, uint64_t first_idx,
                     const uint8_t *bits, size_t count, int32_t *cts);
int eoc_decrypt_bits(const eoc_secret_key *sk, const int32_t *cts, size_t count, uint8_t *bits);
/* Small integers for programmable bootstrapping (eoc_lut_batch_device).
 *   Encoding   m in Z_p, p in {2, 4, 8}, at phase m / (2p) (Torus32 m * 2^32 / (2p)) with the ks_stdev noise of a fresh bit
 *              ciphertext.  The upper half of the torus, [1/2, 1), is a padding half: a phase m / (2p) with m in [p, 2p) is
 *              not a message, and a table lookup maps it to -table[m - p] (negacyclic, X^N = -1).  Ciphertexts add as
 *              int32 arrays (wrapping): x + y encrypts x + y as long as the sum stays below p.
 *   Decryption round(phase * 2p / 2^32) mod p.
 *   Noise      (computed with eoc_tfhe_amd/noise.predict for the default sets and a random key, not measured): output sigma
 *              after the key switch ~0.0042 (Set A) / ~0.0035 (Set B), the mod switch to 2N adds ~0.0022 / ~0.0025; the
 *              decision margin is 1 / (4p):
 *                  p   Set A, one input / sum of two     Set B, one input / sum of two
 *                  2        26 sigma / 20 sigma               29 sigma / 23 sigma
 *                  4        13 sigma / 9.8 sigma              15 sigma / 11 sigma
 *                  8       6.6 sigma / 4.9 sigma             7.3 sigma / 5.7 sigma
 *                 16       3.3 sigma / 2.5 sigma             3.7 sigma / 2.8 sigma
 *              hence p <= 8; p = 16 is refused.  At p = 8 an input that is the SUM of two ciphertexts decodes wrongly
 *              about once in 10^6 lookups on Set A.
 * eoc_encrypt_ints: values[count] (each < p) -> cts[count][n+1]; sample s uses stream (enc_seed, first_idx + s) as
 * eoc_encrypt_bits does.  EOC_ERR_ARG for a p outside {2, 4, 8}, a null pointer or a value >= p (nothing is written). */
int eoc_encrypt_ints(const eoc_secret_key *sk, uint64_t enc_seed, uint64_t first_idx, int p, const uint8_t *values,
                     size_t count, int32_t *cts);
int eoc_decrypt_ints(const eoc_secret_key *sk, int p, const int32_t *cts, size_t count, uint8_t *values);
/* Test polynomial tv[N] of a table: table[m] (m < p) is the Torus32 OUTPUT value for input m -- +-2^29 gives a bit
 * ciphertext (the gates' encoding), k * 2^32 / (2p') an integer in Z_p'.  Rule:
 *   tv[k] = table[round(k p / N)]   for k < N - N / (2p)   (round half up: (k p + N / 2) / N)
 *   tv[k] = -table[0]               for the last N / (2p) coefficients, so that a phase slightly below 0 still gives f(0).
 * A blind rotation by b (the mod-switched phase, in [0, 2N)) leaves tv[b] (b < N) or -tv[b - N] in the constant
 * coefficient: every b within N / (2p) - 1 of m N / p gives table[m] for m < p, and -table[m - p] for m in [p, 2p). */
int eoc_lut_test_polynomial(int p, const int32_t *table, int32_t *tv);
/* Many-LUT test polynomial (eoc_lut_many_batch_device): T = n_tables tables interleaved in one polynomial,
 * tables [T][p] of Torus32 output values as above.  Rule: tv[kT + j] = F_j(kT), F_j(x) = table_j[(x p + N/2) / N] for
 * x < N - N / (2p), -table_j[0] otherwise -- eoc_lut_test_polynomial's rule for table j sampled at x = kT, so that a
 * rotation by any multiple b = kT of T leaves table j's value in coefficient j.  T in {2, 4, 8}, p in {2, 4, 8}, p T <= 16
 * (the coarse mod switch multiplies its noise by T: DESIGN.md 10.1's margins); EOC_ERR_ARG otherwise or for a null pointer. */
int eoc_lut_many_test_polynomial(int p, int n_tables, const int32_t *tables, int32_t *tv);
/* lweSymEncrypt / lwePhase with an arbitrary message and noise (eoc-tfhe-run.cpp:149,161) */
int eoc_lwe_encrypt(const eoc_secret_key *sk, uint64_t enc_seed, uint64_t idx, int32_t mu,
                    double sigma, int32_t *ct);
int32_t eoc_lwe_phase(const eoc_secret_key *sk, const int32_t *ct);
/* worker threads the client-side code uses: min(cores, affinity mask, cgroup quota), or EOC_TFHE_THREADS */
int eoc_host_threads(void);
/* modSwitchToTorus32 / modSwitchFromTorus32 (eoc-tfhe-run.cpp:145,162) */
int32_t eoc_modswitch_to_torus32(int32_t mu, int32_t Msize);
int32_t eoc_modswitch_from_torus32(int32_t phase, int32_t Msize);

/* ------------------------------------------------------------------------------------------------
 * engine API (one engine per GPU; device pointers; asynchronous on `hip_stream`)
 * ---------------------------------------------------------------------------------------------- */
typedef struct eoc_engine eoc_engine;

int eoc_device_count(void);
/* Environment read here, once per engine (INTEGRATION.md section 6 lists every knob; none changes a result).  The slicing ones:
 *   EOC_TFHE_SLICE_SAMPLES = k   the sample rule: at most k extracted samples (blind-rotation jobs) per slice of any device call
 *                                -- table lookups, two-input lookups, a circuit level's job cap, integer circuits, compact
 *                                expansion, table reads, automaton runs, inner products and convolutions.  Default and upper
 *                                limit 2^20 (9.6 GB of workspace); a value outside [1, 2^20] is ignored, so the shipped slices
 *                                cannot be widened.  Diagnostics: tests/test_gpu_slice_seams.py runs every call's second slice
 *                                with it.  The grid limits (32 768 gates, nodes or queries, 65 535 vectors or lists per launch)
 *                                are constants.
 *   EOC_TFHE_INT_SLICE_ROWS, EOC_TFHE_TABLE_WS_BYTES, EOC_TFHE_PACK_WS_BYTES, EOC_TFHE_DOT_WS_BYTES: rows and bytes per slice of
 *                                one family each, described at their calls below. */
int eoc_engine_create(int device, const eoc_params *p, eoc_engine **out);
void eoc_engine_destroy(eoc_engine *e);
const char *eoc_last_error(void);

/* raw HBM buffers for hosts that have no allocator of their own (a Lua/Node host; tests) */
int eoc_device_alloc(eoc_engine *e, size_t bytes, void **d_ptr);
int eoc_device_free(eoc_engine *e, void *d_ptr);
int eoc_host_to_device(eoc_engine *e, void *d_dst, const void *src, size_t bytes);
int eoc_device_to_host(eoc_engine *e, void *dst, const void *d_src, size_t bytes);
int eoc_engine_synchronize(eoc_engine *e);

/* device-side key image sizes in bytes: BK-FFT [n][2l][2][512] complex f64 (bin order sigma, values
 * scaled by 2^-9: the image carries the inverse transform's 1/512, an exact power-of-two scaling),
 * KSK [N*t][base-1][n1p] int32 (rows d = 1..base-1, zero-padded to n1p = eoc_ksk_row_stride) */
size_t eoc_bkfft_bytes(const eoc_params *p);
size_t eoc_ksk_dev_bytes(const eoc_params *p);
size_t eoc_ksk_row_stride(const eoc_params *p);

/* host torus-form keys -> device images (H2D, pad KSK, forward-transform BK on the GPU).
 * Replaces new_LweBootstrappingKeyFFT / tGswToFFTConvert.  Synchronous. */
int eoc_engine_load_cloud_key(eoc_engine *e, const int32_t *bk, const int32_t *ksk);
/* same, written into caller-owned device buffers of eoc_bkfft_bytes / eoc_ksk_dev_bytes, which the
 * engine then uses (not freed by the engine) */
int eoc_engine_build_cloud_key_device(eoc_engine *e, const int32_t *bk, const int32_t *ksk,
                                      void *d_bkfft, void *d_ksk);
/* adopt caller-owned device images (e.g. buffers filled by an RCCL broadcast); not freed by the
 * engine; must stay valid while the engine uses them.  The images must be COMPLETE when they are installed (here and in
 * eoc_engine_adopt_cloud_key_device): the engine derives its own int8-limb image of the key-switch key from d_ksk in this
 * call (it drains the device first) and does not look at d_ksk's later changes until a key is installed again. */
int eoc_engine_set_cloud_key_device(eoc_engine *e, const void *d_bkfft, const void *d_ksk);
/* take OWNERSHIP of device images allocated with eoc_device_alloc on this engine (key replicas filled by a
 * broadcast or a peer copy); the engine frees them */
int eoc_engine_adopt_cloud_key_device(eoc_engine *e, void *d_bkfft, void *d_ksk);
/* borrow the engine's images (for broadcasting them, or for parity checks) */
int eoc_engine_cloud_key_device(eoc_engine *e, const void **d_bkfft, const void **d_ksk);

/* Concurrency: calls on one engine are serialised by a mutex and share one workspace set, so an engine must be
 * driven from ONE stream at a time (launches of successive calls on the same stream are ordered; use one
 * engine per stream, or synchronise, if several streams are needed).  Workspaces (device buffers and the pinned
 * host ring that carries gate descriptors) grow on demand outside the kernels (device synchronise + hipMalloc);
 * eoc_engine_reserve sizes them once, after which the launch path does not allocate and a fixed
 * netlist / batch shape can be captured into a hipGraph.  eoc_engine_workspace_grows counts growths since the
 * last reserve (0 in steady state).  It synchronises in ONE place: when the descriptor ring (max_descs slots, at least
 * 1 024) wraps around -- a batch of one two-input opcode sends its descriptor as a kernel argument and never uses the
 * ring; MUX batches, mixed batches and circuits consume one slot per gate and level -- the call waits, on an event recorded behind the
 * engine's own most recent kernels, until the slots it is about to rewrite have been consumed.  Only this engine's
 * earlier work is waited for (no device-wide synchronise: a neighbouring batch's copy streams and captures on other
 * streams are not touched); a call on a capturing stream never wraps (its descriptors go to the arena below).
 * Capture rules: call eoc_engine_reserve BEFORE any stream of the process starts capturing -- growth synchronises the
 * whole device, which invalidates a global-mode capture in progress on ANY stream, and only the stream passed to the
 * call can be tested for it.  While hip_stream itself is being captured a call that would have to grow the workspace
 * fails with EOC_ERR_STATE (nothing may be allocated under capture); gate descriptors -- and the opcode permutation of a mixed
 * batch with more than 15 opcode runs -- are placed in an arena that is never re-used (4 x max_descs slots of 40 bytes;
 * a permutation takes count / 10 slots), because the captured copy nodes read their pinned sources again at every
 * replay; when the arena is exhausted the call fails with EOC_ERR_STATE.
 *   max_jobs       : blind rotations of the widest level (instances x gates of the level, MUX counts twice; in a mixed
 *                    batch ALL bootstrapped rows of the call share one pooled blind rotation -- rows with two-input opcodes
 *                    + 2 x MUX rows -- unless that exceeds 2^20 jobs, beyond which every opcode group is a level of its own)
 *   max_descs      : gate descriptors sent between two wrap-arounds of the ring (>= gates of the netlist)
 *   max_mixed_rows : rows of the largest mixed (ops != NULL) batch, 0 if none */
int eoc_engine_reserve(eoc_engine *e, size_t max_jobs, size_t max_descs, size_t max_mixed_rows);
uint64_t eoc_engine_workspace_grows(eoc_engine *e);
/* k_blind_rotate kernel launches so far (eoc_engine_kernel_times counts one span per blind-rotate CALL; a wide level is
 * cut into single-round launches and a gadget-length-3 blind rotation into two parts, so launches >= spans) */
uint64_t eoc_engine_blind_rotate_launches(eoc_engine *e);
/* ... of which launches of the one-wave-per-ciphertext kernel (k_blind_rotate_wide, gadget length 2; bit-identical to the
 * pair kernel, tests/test_gpu_parity.py).  The shipped rule: a level of more than 4 x CUs blind rotations (1 024 on MI355X)
 * runs as full wide launches of 8 x CUs (2 048) and a remainder, which runs wide when it exceeds 4 x CUs and on the pair
 * kernel otherwise; a level of at most 4 x CUs runs on the pair kernel */
uint64_t eoc_engine_blind_rotate_wide_launches(eoc_engine *e);
/* key-switch launches that ran on the matrix cores (k_keyswitch_mfma: basebit 2, t 8, i.e. both default sets; exact int8-limb
 * products, the same words as the look-up kernel -- tests/test_gpu_ks_mfma.py).  EOC_TFHE_KS_MFMA=0|1 forces either form. */
uint64_t eoc_engine_keyswitch_mfma_launches(eoc_engine *e);
/* blind rotations that fill the device in ONE launch: 8 x compute units where the one-wave-per-ciphertext kernel applies
 * (gadget length 2), 4 x otherwise.  A host that cuts a long job into pieces should cut at multiples of this (the
 * host-buffer batch path does). */
size_t eoc_engine_resident_jobs(eoc_engine *e);
int eoc_engine_device(eoc_engine *e);
const eoc_params *eoc_engine_params(eoc_engine *e);
/*
 * one homogeneous or mixed batch of independent gates, all operands resident on the device.
 *   op      : opcode when ops == NULL
 *   ops     : HOST array [count] of opcodes in any order, or NULL (rows are grouped on the device: gather into
 *             opcode-sorted order; the ten two-input opcodes -- which differ only in their linear stage -- form one
 *             group, MUX rows another, and both share ONE blind rotation over the concatenated jobs; NOT / COPY /
 *             CONSTANT take no bootstrap; scatter back).  At most 2^28 - 1 rows per call with ops != NULL (EOC_ERR_ARG
 *             beyond)
 *   d_in*   : DEVICE arrays [count][n+1] int32 (d_in1 unused by NOT/COPY, d_in2 only by MUX, MAJ and XOR3)
 *   d_out   : DEVICE array  [count][n+1] int32
 * bootsNAND ... bootsMUX over a batch.  Asynchronous on hip_stream (NULL = default stream). */
int eoc_gate_batch_device(eoc_engine *e, int op, const uint8_t *ops, const int32_t *d_in0,
                          const int32_t *d_in1, const int32_t *d_in2, int32_t *d_out, size_t count,
                          void *hip_stream);

/* netlist evaluation: `instances` independent copies of one circuit.
 * wires: DEVICE array [n_wires][instances][n+1]; gate g reads wires in0,in1,in2 and writes out.
 * Gates must be topologically ordered; the engine levelises them (read-after-write, write-after-read and write-after-write
 * hazards on wires: a netlist may re-use wires) and batches every level over all instances: one blind rotation for all
 * bootstrapped gates of a level, preceded by one pre-pass for its free gates -- NOT / COPY / CONSTANT cost no level. */
typedef struct eoc_gate {
    int32_t op;
    int32_t in0, in1, in2; /* wire ids (unused = -1) */
    int32_t out;
} eoc_gate;
int eoc_circuit_run_device(eoc_engine *e, const eoc_gate *gates, size_t n_gates, int32_t *d_wires,
                           size_t n_wires, size_t instances, void *hip_stream);
/* number of bootstraps (blind rotations) a netlist costs per instance: MUX = 2, NOT / COPY / CONSTANT = 0, everything else 1 */
size_t eoc_circuit_bootstraps(const eoc_gate *gates, size_t n_gates);
/* Netlist rewriting on the host (no GPU), four passes repeated until nothing changes:
 *   duplicates  a gate that repeats an earlier one (same opcode, same wires, operand order aside where the gate is symmetric)
 *               becomes a COPY of it; a gate that reads one wire twice is no gate (AND(x, x) = x, XOR(x, x) = 0, MUX(s, b, b) = b,
 *               MUX(s, s, c) = OR(s, c), MAJ(x, x, y) = x, ...).  Sharing a wire can take a single-use wire away from a later
 *               pattern: the pipeline runs with and without this pass and the better result is returned (fewest bootstraps,
 *               then levels, then gates)
 *   constants   bootsCONSTANT wires are folded into their readers (AND(x, 0) = 0, XOR(x, 1) = NOT x, MUX(s, 0, c) = ANDNY(s, c),
 *               MUX(s, b, 1) = ORNY(s, b), ...: a MUX with a known branch costs one bootstrap instead of two)
 *   NOT / COPY  folded into their readers (the ten two-input gates are closed under input negation; a negated MUX selector
 *               swaps the branches; NOT(NOT x) = COPY; every reader looks through COPY)
 *   MUX fusion  OR(AND(s, b), ANDNY(s, c)) with single-use inner wires -> MUX(s, b, c)
 *   carry       OR(AND(a, b), AND(XOR(a, b), c)) (the second AND single-use) -> MUX(XOR(a, b), c, a): the textbook full adder's
 *               carry as ONE gate on ONE level (the literal 8-bit ripple-carry adder: 40 bootstraps / 17 levels -> 30 / 8)
 * and gates nobody reads are dropped.  `outputs` are the wires the caller reads afterwards.  Input slots an opcode does not
 * use are ignored whatever they hold (and come back as -1); wire ids must be below 2^24.  Single-assignment netlists
 * only (every wire written at most once, after its readers' inputs): otherwise EOC_ERR_ARG.  gates_out has room for n_gates
 * entries; returns the number of gates written.  Same wire numbering, never more bootstraps, never more levels. */
int64_t eoc_netlist_optimize(const eoc_gate *gates, size_t n_gates, const int32_t *outputs, size_t n_outputs,
                             eoc_gate *gates_out);
/* ... with flags.  By default (flags 0, = eoc_netlist_optimize) the rewriting may use the EXTENSION gates: the full adder's
 * carry becomes EOC_MAJ(a, b, c) (one bootstrap, not MUX's two); a MUX whose selector is XOR / XNOR(x, y) and one of whose
 * branches is x or y becomes a majority -- MUX(XOR(x, y), c, x) = EOC_MAJ(x, y, c), the borrow / comparator step
 * MUX(XNOR(a, b), lt, b) = EOC_MAJ(NOT a, b, lt) with the NOT on the selector's wire once that has no other reader -- and
 * XOR(XOR(a, b), c) whose inner wire then dies becomes EOC_XOR3(a, b, c): the literal 8-bit ripple-carry adder goes from 40
 * bootstraps on 17 levels to 16 on 8, the textbook subtractor from 30 to 16, the comparator chain from 22 to 8.
 * EOC_NL_BOOTS_GATES_ONLY keeps the result inside libtfhe's boots* family (the carry as MUX: 30 bootstraps on 8 levels). */
enum { EOC_NL_BOOTS_GATES_ONLY = 1 };
int64_t eoc_netlist_optimize_ex(const eoc_gate *gates, size_t n_gates, const int32_t *outputs, size_t n_outputs,
                                eoc_gate *gates_out, unsigned flags);
/* levels of a netlist exactly as eoc_circuit_run_device assigns them (RAW, WAR, WAW hazards; 1-based; level_of[n_gates] or
 * NULL; a free gate carries the level in whose pre-pass it runs); *bootstrap_levels (or NULL) = levels that hold at least
 * one blind rotation -- the sequential depth a small batch pays for.  Returns the number of levels. */
int64_t eoc_netlist_levels(const eoc_gate *gates, size_t n_gates, int32_t *level_of, int64_t *bootstrap_levels);
/* Estimated run time of a netlist over `instances` instances, in units of 0.1 ms on one MI355X (Set A): a level of
 * J = instances x jobs blind rotations runs as J / R full launches (3.0 ms) plus one partly filled launch costing
 * 1.4 ms + 1.6 ms x max(J mod R, R / 4) / R (measured: 1.8 / 2.3 / 3.0 ms at 256 / 512 / 1024 gates; R = resident_jobs, 0 =
 * 1024 = four ciphertexts per compute unit).  Below R / 4 a level costs the same whatever its width: DEPTH is the cost of a
 * small batch, BOOTSTRAPS that of a large one -- what the facades' addBits / lessThanBits use to pick a circuit form
 * (ripple / MUX-carry / parallel-prefix) for an instance count.  No GPU needed. */
int64_t eoc_netlist_cost(const eoc_gate *gates, size_t n_gates, size_t instances, size_t resident_jobs);

/* building blocks exposed for parity tests and profiling (device pointers, async) */
int eoc_dbg_fft_fwd_device(eoc_engine *e, const int32_t *d_polys, double *d_specs, size_t count,
                           void *hip_stream);
/* CONVERSION CONTRACT of the inverse transform -- here and inside every blind rotation (tLweFromFFTConvert /
 * TorusPolynomial_fft): each value v is converted as Torus32(int64(v)), truncation toward zero then
 * wrap mod 2^32, FOR |v| < 2^51.  The device uses two exact operations (trunc, then + 1.5 * 2^52 and the low dword),
 * which equal the int64 conversion on that range only; for 2^51 <= |v| < 2^52 the result is the two-operation form's
 * (defined, pinned by tests/test_gpu_parity.py::test_conversion_contract_pinned_around_2_pow_51), not int64's.
 * Reach: an external-product coefficient is bounded by l * Bg * 2^41 -- below 2^51, i.e. the contract holds
 * UNCONDITIONALLY, iff l * Bg < 1024 (Set B: 384; every shape with l * Bg that small).  Set A (l * Bg = 2048) has the
 * exact bound 2^52; |v| >= 2^51 there needs all 4096 digit x key products aligned and has probability <= 2 e^-512 per
 * coefficient for any digit vector (Hoeffding on the independent uniform mask coefficients); real
 * bootstraps stay near 2^45. */
int eoc_dbg_fft_inv_device(eoc_engine *e, const double *d_specs, int32_t *d_polys, size_t count,
                           void *hip_stream);
/* t[count][n+1] -> u[count][N+1]  (tfhe_blindRotateAndExtract_FFT, mu = 1/8) */
int eoc_blind_rotate_device(eoc_engine *e, const int32_t *d_t, int32_t *d_u, size_t count,
                            void *hip_stream);
/* u[count][N+1] -> out[count][n+1]  (lweKeySwitch) */
int eoc_keyswitch_device(eoc_engine *e, const int32_t *d_u, int32_t *d_out, size_t count,
                         void *hip_stream);
/* Programmable bootstrapping: table lookups on small integers (encoding and noise: eoc_encrypt_ints above).
 *   d_tv   DEVICE array [n_luts][N] of test polynomials (eoc_lut_test_polynomial), 1 <= n_luts <= 32 768
 *   d_in   DEVICE array [count][n+1] of input samples
 *   d_out  DEVICE array [n_luts][count][n+1]: out[t][r] = KeySwitch(BlindRotate(in[r], tv[t]))
 * Every table is applied to every row in ONE level of n_luts x count blind rotations (k_prepare, the blind rotation, the key
 * switch), so that one input yields several functions of itself -- a value and its carry, say -- for the depth of one
 * bootstrap.  The blind rotation is the gate kernel's with its accumulator seeded from the job's test polynomial
 * (k_blind_rotate_tv / k_blind_rotate_wide_tv); shapes and segmentation are those of a gate level of the same job count.
 * Workspace and capture rules: those of eoc_engine_reserve above, with max_jobs = n_luts x count (a call of more than
 * 2^20 jobs runs as several levels of at most 2^20 jobs and needs max_jobs = that slice) and max_descs >= n_luts.
 * Asynchronous on hip_stream.  EOC_ERR_ARG for a null pointer or n_luts outside [1, 32 768]. */
int eoc_lut_batch_device(eoc_engine *e, const int32_t *d_tv, size_t n_luts, const int32_t *d_in, int32_t *d_out,
                         size_t count, void *hip_stream);
/* Many-LUT bootstrapping: T = n_tables functions of every row from ONE blind rotation.
 *   d_tv   DEVICE array [n_luts][N] of packed test polynomials (eoc_lut_many_test_polynomial), T tables each
 *   d_in   DEVICE array [count][n+1] of input samples (eoc_encrypt_ints encoding, p T <= 16)
 *   d_out  DEVICE array [n_luts][T][count][n+1]: out[g][j][r] = table j of polynomial g applied to row r
 * One level per row slice: the mod switch to multiples of T (k_modswitch_coarse), n_luts x count blind rotations through the
 * gate levels' launch policy (k_lut_many / k_lut_many_wide: the _tv kernels' prologue and step loop, T extractions), then
 * the key switch of n_luts x T x count samples.  Output noise is the gate bootstrap's.  Stats: bootstraps += n_luts x count,
 * keyswitches += n_luts x T x count.
 * Workspace and capture rules: those of eoc_engine_reserve, with max_jobs = n_luts x T x rows of a slice (a slice holds at
 * most 2^20 extracted samples: rows = min(count, 2^20 / (n_luts T))) and max_descs >= n_luts x (T + 1) per slice.
 * Asynchronous on hip_stream.  EOC_ERR_ARG for a null pointer, T outside {2, 4, 8} or n_luts x T outside [1, 32 768]. */
int eoc_lut_many_batch_device(eoc_engine *e, int n_tables, const int32_t *d_tv, size_t n_luts, const int32_t *d_in,
                              int32_t *d_out, size_t count, void *hip_stream);
/* Integer circuits: netlists of linear stages and table lookups.  A node forms
 *   t = sum_k w[k] wire[in[k]] + (0, ..., 0, cst)        wrapping int32, word by word over the n + 1 words of a sample
 * and writes
 *   n_tables == 0          out = t                                    a FREE node: no bootstrap
 *   n_tables == 1          out = KeySwitch(BlindRotate(modswitch(t), tv))    what eoc_lut_batch_device gives for a row t
 *   n_tables == T in 2,4,8 wires out .. out + T - 1 = the T outputs eoc_lut_many_batch_device gives for a row t (the mod
 *                          switch rounds onto the T-grid; output j goes to wire out + j)
 * The netlist is single-assignment and topologically ordered: every wire is written by at most one node, and a node reads
 * only wires that no node writes (the circuit's inputs) or outputs of EARLIER nodes.  Wires are laid out
 * [wire][instance][n+1], as in eoc_circuit_run_device.  Entries of in[] / w[] from n_terms on are ignored.
 * Levels: a bootstrapped node sits one level above the deepest bootstrapped producer among its inputs (inputs: level 0); a
 * free node costs no level: it runs in the pre-pass of the level after its deepest producer (level_of = that level, which
 * is n_levels + 1 -- the last pre-pass -- when nothing bootstrapped follows it).
 * Message ranges and noise are the caller's to track: eoc_tfhe_amd.IntCircuit.check does both. */
#define EOC_INODE_MAX_TERMS 4
typedef struct {
    int32_t n_tables; /* 0: linear node, no bootstrap (free); 1: one table; 2, 4, 8: many-LUT, T outputs */
    int32_t out;      /* output wire; a many-LUT node writes wires out .. out + T - 1 */
    int32_t tv;       /* index of the node's test polynomial in d_tv[n_tv][N]; ignored when n_tables == 0 */
    int32_t n_terms;  /* 1 .. EOC_INODE_MAX_TERMS */
    int32_t in[EOC_INODE_MAX_TERMS];
    int32_t w[EOC_INODE_MAX_TERMS];  /* integer weights */
    int32_t cst;      /* Torus32 constant added to b */
} eoc_inode;
/* Host only, no GPU: validates the netlist and returns its number of bootstrap levels (>= 0).  level_of [n_nodes] and
 * bootstraps may be NULL; *bootstraps = blind rotations per instance (one per node with n_tables >= 1).  EOC_ERR_ARG for a
 * null netlist with n_nodes > 0, a wire or tv index out of range, n_terms outside [1, 4], n_tables not in {0, 1, 2, 4, 8},
 * a many-LUT node whose out + T exceeds n_wires, a wire written twice, or a node that reads a wire written by itself or by
 * a later node. */
int64_t eoc_int_netlist_levels(const eoc_inode *nodes, size_t n_nodes, size_t n_wires, size_t n_tv, int32_t *level_of,
                               int64_t *bootstraps);
/* Runs the netlist over `instances` rows of every wire: d_tv DEVICE [n_tv][N] test polynomials (eoc_lut_test_polynomial
 * for a node with one table, eoc_lut_many_test_polynomial for T tables), d_wires DEVICE [n_wires][instances][n+1].
 * Per level and per slice of rows: one k_lin_modswitch launch for the level's free nodes, then per group of nodes with equal
 * T one k_lin_modswitch launch (linear stage + mod switch onto the T-grid: the rotation amounts), ONE blind rotation over
 * all of the group's nodes x rows through the gate levels' launch policy (k_blind_rotate_tv / k_lut_many families), and one
 * key switch over the group's outputs.  Results equal eoc_lut_batch_device / eoc_lut_many_batch_device on rows t, bit for
 * bit.  Stats: bootstraps += bootstrapped nodes x instances, keyswitches += their outputs x instances.
 * Slices: a group holds at most 2^20 extracted samples (rows = min(instances, 2^20 / the widest group's outputs)).
 * Workspace and capture rules: those of eoc_engine_reserve, with max_jobs = the widest group's outputs x rows of a slice,
 * max_descs >= 2 (nodes + outputs) + 64 and max_mixed_rows >= bootstrapped nodes x N / (4 (n + 1)) + 1 (the nodes' test
 * polynomials are gathered into level order once per call, in the mixed-batch area).
 * Asynchronous on hip_stream.  EOC_ERR_ARG as eoc_int_netlist_levels and for a null pointer, before anything touches the
 * device; EOC_ERR_NO_KEY without a cloud key; n_nodes = 0 or instances = 0 is a no-op. */
int eoc_int_circuit_run_device(eoc_engine *e, const eoc_inode *nodes, size_t n_nodes, const int32_t *d_tv, size_t n_tv,
                               int32_t *d_wires, size_t n_wires, size_t instances, void *hip_stream);
/* Compact public-key lists -> LWE samples (formats and security: "compact public-key encryption" below).
 *   d_lists  DEVICE array [ceil(count / N)][2][N] int32 of lists (eoc_pk_encrypt_*): sample s is slot s mod N of list s / N
 *   d_out    DEVICE array [count][n+1]: out[s] = lweKeySwitch(extract(list s / N, slot s mod N)) with the engine's KSK
 * Extraction of slot j: a'_i = c0[j - i] (i <= j), -c0[N + j - i] (i > j), b' = c1[j] -- an LWE sample of dimension N under
 * the TLWE key s', which the key-switch key takes to the LWE key.  Both steps are integer operations: the result equals the
 * CPU composition (orc_keyswitch of the extracted sample) bit for bit.  One extraction kernel (k_compact_expand) writes the
 * key switch's operand rows, then the key switch runs unchanged; calls run in slices of at most 2^20 samples.  Needs the KSK
 * only (EOC_ERR_NO_KEY without one); stats: keyswitches += count.  Workspace and capture rules: those of eoc_engine_reserve,
 * with max_jobs = min(count, 2^20) (no descriptor slot is used).  Asynchronous on hip_stream.  EOC_ERR_ARG for a null
 * pointer; count 0 is a no-op. */
int eoc_compact_expand_device(eoc_engine *e, const int32_t *d_lists, size_t count, int32_t *d_out, void *hip_stream);
/* per-kernel timing with HIP events recorded on the launch stream.  kinds: [0] prepare,
 * [1] blind_rotate, [2] keyswitch.  eoc_engine_kernel_times synchronises the device. */
int eoc_engine_set_profiling(eoc_engine *e, int on);
int eoc_engine_kernel_times(eoc_engine *e, double ms[3], uint64_t launches[3], int reset);
/* last launch statistics: kernel names/grids are in the rocprof trace; this returns counters the
 * host keeps: [0] batches, [1] bootstraps, [2] keyswitches */
int eoc_engine_stats(eoc_engine *e, uint64_t out[3]);

/* ------------------------------------------------------------------------------------------------
 * batch API (host buffers; synchronous: H2D, kernels, D2H) on the process-global GPU context: ONE host process and
 * ONE key -- the reference's globalSecretKey / globalPublicKey (ao-tfhe/eoc-tfhe-run.cpp:38-40) behind the
 * luaopen_tfhe registry (ao-tfhe/eoc-tfhe-bindings.c:128-148) -- in front of ANY number of GPUs.
 *   eoc_gpu_init_multi   one engine per listed device (a device may be listed more than once: several engines then
 *                        share it, which is how a one-GPU box rehearses the N-GPU path)
 *   eoc_gpu_init         = eoc_gpu_init_multi(&device, 1, p)
 *   eoc_gpu_init_from_env  devices from eoc_gpu_set_devices if that was called, else EOC_TFHE_DEVICES = "all" |
 *                        "0,1,2,..." (unset: device 0); what the string API uses when a gate key arrives, so a Lua /
 *                        Node host scales without changing its calls
 *   eoc_gpu_set_devices  remembers a device list for that bring-up (n_devices 0 forgets it); no GPU is touched
 *   eoc_upload_cloud_key the two key images are built once on the first device and replicated: ncclBroadcast over
 *                        xGMI (librccl, loaded on demand) when the devices are distinct, device-to-device / peer copies
 *                        otherwise (EOC_TFHE_KEY_BCAST = rccl | copy forces one).  Keys are replicated, never sharded.
 *   eoc_gate_batch / eoc_circuit_run  cut their instances into contiguous blocks (eoc_shard_range: blocks differ by at
 *                        most one, the same blocks as eoc_tfhe_amd.distributed.shard), one block per engine, one host
 *                        thread per engine; a whole circuit instance stays on one device; no data-path collective.
 *                        Per device: persistent device buffers; operands in buffers from eoc_host_alloc (pinned,
 *                        device-mapped) are read in place by the first kernel, pageable ones are copied.
 * ---------------------------------------------------------------------------------------------- */
int eoc_gpu_init(int device, const eoc_params *p);
int eoc_gpu_init_multi(const int *devices, int n_devices, const eoc_params *p);
int eoc_gpu_init_from_env(const eoc_params *p);
int eoc_gpu_set_devices(const int *devices, int n_devices);
int eoc_gpu_engine_count(void);
int eoc_upload_cloud_key(const eoc_secret_key *sk);    /* push sk's BK/KSK to every engine of the global context */
int eoc_upload_cloud_key_arrays(const int32_t *bk, const int32_t *ksk); /* same from raw torus-form arrays */
eoc_engine *eoc_global_engine(void);                   /* engine 0 */
eoc_engine *eoc_global_engine_at(int i);
void eoc_gpu_shutdown(void);
int eoc_stats(uint64_t out[3]);                        /* eoc_engine_stats summed over the engines */
/* per_device[engines][3] counters; returns the number of engines; key replication time and method */
int eoc_stats_multi(uint64_t *per_device, int cap_devices, double *key_broadcast_seconds);
const char *eoc_key_broadcast_method(void);            /* "rccl" | "peer-copy" | "none" */
uint64_t eoc_host_path_buffer_grows(void);             /* growths of the persistent I/O buffers (0 in steady state) */
/* where the RCCL used by the key broadcast came from: "not loaded" | "already mapped" (the process had one, e.g. a
 * torch-hosting harness: re-used, never a second copy) | "process symbols" | the name it was dlopen'ed under */
const char *eoc_rccl_origin(void);
/* one-GPU rehearsal of the RCCL call path of the key broadcast: one-rank communicator on `device` (ncclCommInitAll), a
 * grouped out-of-place ncclBroadcast of `bytes` bytes (0 = 1 MiB) through the dlopen'ed table, result compared */
int eoc_rccl_selftest(int device, size_t bytes);
/* Engines 1..n-1 each have ONE persistent host thread (engine 0's block runs on the calling thread); a call wakes only
 * the threads whose block of the call is non-empty.  Wake-ups of engine i's thread since eoc_gpu_init_multi (0 for i = 0) */
uint64_t eoc_worker_wakeups(int engine_index);
void eoc_shard_range(size_t total, int rank, int world, size_t *lo, size_t *hi);
/* Asynchronous form of eoc_gate_batch: returns once the batch is queued (operands on the H2D stream, kernels behind
 * them, results on the D2H stream).  Every buffer must come from eoc_host_alloc and stay untouched until
 * eoc_gate_batch_wait(ticket).  Two submissions may be in flight (a third first waits for the oldest); they execute in
 * submission order; a host that keeps two in flight hides one batch's PCIe time behind the other's kernels.  Every
 * synchronous call on the global context drains pending submissions first.  `ops` is read during the call. */
int eoc_gate_batch_submit(int op, const uint8_t *ops, const int32_t *in0, const int32_t *in1, const int32_t *in2,
                          int32_t *out, size_t count, uint64_t *ticket);
int eoc_gate_batch_wait(uint64_t ticket);
/* pinned host memory for I/O buffers of the batch API (true DMA, chunked overlap); release with eoc_host_free */
void *eoc_host_alloc(size_t bytes);
void eoc_host_free(void *p);
int eoc_gate_batch(int op, const uint8_t *ops, const int32_t *in0, const int32_t *in1,
                   const int32_t *in2, int32_t *out, size_t count);
int eoc_circuit_run(const eoc_gate *gates, size_t n_gates, int32_t *wires, size_t n_wires,
                    size_t instances);
/* Table lookups on the global context (host buffers, synchronous): tables [n_luts][p] of Torus32 output values (see
 * eoc_lut_test_polynomial), in [count][n+1] encrypted at message space p (eoc_encrypt_ints), out [n_luts][count][n+1].
 * Rows are cut into eoc_shard_range blocks, one per engine, as eoc_gate_batch does; the cloud key alone suffices (a
 * server context).  EOC_ERR_ARG for p outside {2, 4, 8}, n_luts = 0 or a null pointer. */
int eoc_lut_batch(int p, const int32_t *tables, size_t n_luts, const int32_t *in, int32_t *out, size_t count);
/* Many-LUT lookups on the global context (host buffers, synchronous): tables [n_luts][T][p] (eoc_lut_many_test_polynomial
 * builds one polynomial per n_luts entry on the host), in [count][n+1], out [n_luts][T][count][n+1].  Rows are sharded per
 * engine as in eoc_lut_batch; the cloud key alone suffices.  EOC_ERR_ARG for an unsupported (p, T), n_luts = 0 or a null
 * pointer. */
int eoc_lut_many_batch(int p, int n_tables, const int32_t *tables, size_t n_luts, const int32_t *in, int32_t *out,
                       size_t count);
/* Integer circuit on the global context (host buffers, synchronous): the netlist of eoc_int_circuit_run_device with its
 * tables as Torus32 output values.  Entry i of the n_tv entries has table_T[i] tables of table_p[i] values each, stored
 * one entry after the other in `tables` ([T_0][p_0], then [T_1][p_1], ...); its polynomial is built on the host with
 * eoc_lut_test_polynomial (T_i = 1) or eoc_lut_many_test_polynomial.  wires [n_wires][instances][n+1] in host memory: the
 * input wires' rows are read, every written wire's rows are filled in.  Instances are cut into eoc_shard_range blocks,
 * one per engine; the cloud key alone suffices.  EOC_ERR_ARG as eoc_int_netlist_levels, for an unsupported (p_i, T_i)
 * and for a null pointer. */
int eoc_int_circuit_run(const eoc_inode *nodes, size_t n_nodes, const int32_t *tables, const int32_t *table_p,
                        const int32_t *table_T, size_t n_tv, int32_t *wires, size_t n_wires, size_t instances);

/* ------------------------------------------------------------------------------------------------
 * string API (reference style; global key context)
 * ---------------------------------------------------------------------------------------------- */
/* like generateSecretKey (eoc-tfhe-run.cpp:214-250) but for the Boolean path: creates the global
 * secret + cloud key, brings up the GPU engine and uploads the cloud key.  seed = 0: secure mode (getrandom +
 * ChaCha20); any other seed: the reproducible test mode (NOT secure).  Returns a short base64 token describing
 * the key (params + seed), NULL if a key already exists (eoc-tfhe-run.cpp:245-249) or on error. */
const char *generateGateKey(int minimum_lambda, uint64_t seed);
void resetGateKey(void);
/* bootsSymEncrypt / bootsSymDecrypt on base64(export_lweSample_toStream bytes):
 * little-endian a[n] | b | f64 current_variance  (eoc-tfhe-run.cpp:293-295) */
const char *encryptBit(int bit, const char *base64SecretKey);
/* bootsCONSTANT as a string: the noiseless trivial sample of `bit` (no key material involved, variance 0) */
const char *constantBit(int bit);
int decryptBit(const char *base64Ciphertext, const char *base64SecretKey);
/* boots* gates, signature style of addCiphertexts (eoc-tfhe-run.cpp:427) */
const char *gateNAND(const char *ct1, const char *ct2, const char *base64PublicKey);
const char *gateAND(const char *ct1, const char *ct2, const char *base64PublicKey);
const char *gateOR(const char *ct1, const char *ct2, const char *base64PublicKey);
const char *gateNOR(const char *ct1, const char *ct2, const char *base64PublicKey);
const char *gateXOR(const char *ct1, const char *ct2, const char *base64PublicKey);
const char *gateXNOR(const char *ct1, const char *ct2, const char *base64PublicKey);
const char *gateNOT(const char *ct1, const char *base64PublicKey);
const char *gateMUX(const char *ct1, const char *ct2, const char *ct3, const char *base64PublicKey);
/* the extension gates (EOC_MAJ, EOC_XOR3), signature style of gateMUX */
const char *gateMAJ(const char *ct1, const char *ct2, const char *ct3, const char *base64PublicKey);
const char *gateXOR3(const char *ct1, const char *ct2, const char *ct3, const char *base64PublicKey);

/* ------------------------------------------------------------------------------------------------
 * f1: the reference's own 11 calls, same symbols and signatures (ao-tfhe/eoc-tfhe-run.h:8-19,
 * ao-tfhe/eoc-tfhe-run.cpp:167-513).  Wide-message LWE (Msize = 2^31-1), CPU work as in the reference.
 * generateSecretKey uses minimum_lambda = 128 (Set B) and returns the compact key blob below.
 * ---------------------------------------------------------------------------------------------- */
const char *generateSecretKey(const char *jwtToken, const char *jwksBase64);
const char *generatePublicKey(); /* declared but never defined by the reference (eoc-tfhe-run.h:10); here = exportCloudKey() */
const char *encryptInteger(int32_t value, const char *base64SecretKey);
const char *encryptInteger_dummy(int32_t value, const char *base64SecretKey);
const int decryptInteger(char *base64Ciphertext, const char *base64SecretKey, const char *jwtToken,
                         const char *jwksBase64);
const char *addCiphertexts(const char *base64Ciphertext1, const char *base64Ciphertext2,
                           const char *base64PublicKey);
const char *subtractCiphertexts(const char *base64Ciphertext1, const char *base64Ciphertext2,
                                const char *base64PublicKey);
const char *encrypt8BitASCIIString(const char *text, const int16_t msgLength, const char *base64Key);
const char *decrypt8BitASCIIString(char *base64Ciphertext, const int16_t msgLength, const char *base64Key,
                                   const char *jwtToken, const char *jwksBase64);
void info(void);
void testJWT();

/* ------------------------------------------------------------------------------------------------
 * f2: key export / import (the reference exports at eoc-tfhe-run.cpp:235-243 but has no import
 * path).  Versioned flat little-endian formats:
 *   secret key "EOCSK1": params | seed | lwe bits | tlwe bits  (reproducible keys; the cloud key is regenerated
 *                        from the seed; import verifies the key bits)
 *              "EOCSK2": params | 256-bit master key | lwe bits | tlwe bits  (secure keys, same idea)
 *   cloud key  "EOCCK1": params | bk int32[] | ksk int32[]      (what a server needs; no secrets)
 * ---------------------------------------------------------------------------------------------- */
size_t eoc_secret_key_export(const eoc_secret_key *sk, void *buf, size_t cap); /* returns bytes needed */
int eoc_secret_key_import(const void *buf, size_t len, int with_cloud_key, eoc_secret_key **out);
size_t eoc_cloud_key_blob_bytes(const eoc_params *p);
int eoc_cloud_key_export(const eoc_secret_key *sk, void *buf, size_t cap);
int eoc_cloud_key_blob_params(const void *buf, size_t len, eoc_params *p);
int eoc_engine_create_from_cloud_key_blob(int device, const void *buf, size_t len, eoc_engine **out);
/* raw-buffer calls on the GLOBAL key (what a Node/Lua batch wrapper uses instead of base64 strings); the
 * gate calls bring the GPU engine up on first use and fail without a GPU */
int eoc_global_params(eoc_params *out);
int eoc_global_encrypt_bits(const uint8_t *bits, size_t count, int32_t *cts);
int eoc_global_decrypt_bits(const int32_t *cts, size_t count, uint8_t *bits);
/* eoc_encrypt_ints / eoc_decrypt_ints on the global key (secure-mode randomness, as eoc_global_encrypt_bits) */
int eoc_global_encrypt_ints(int p, const uint8_t *values, size_t count, int32_t *cts);
int eoc_global_decrypt_ints(int p, const int32_t *cts, size_t count, uint8_t *values);
int eoc_global_gate_batch_submit(int op, const uint8_t *ops, const int32_t *in0, const int32_t *in1,
                                 const int32_t *in2, int32_t *out, size_t count, uint64_t *ticket);
int eoc_global_gate_batch(int op, const uint8_t *ops, const int32_t *in0, const int32_t *in1,
                          const int32_t *in2, int32_t *out, size_t count);
int eoc_global_circuit_run(const eoc_gate *gates, size_t n_gates, int32_t *wires, size_t n_wires,
                           size_t instances);
const char *exportSecretKey(void);          /* base64 of the EOCSK1 blob of the global key */
int importSecretKey(const char *base64Key); /* 0, or -1 (malformed / a key already exists) */

/* ------------------------------------------------------------------------------------------------
 * f2, server side: the cloud ("public") key on the global context.  The reference aliases the cloud key set of its
 * secret key as globalPublicKey (ao-tfhe/eoc-tfhe-run.cpp:232-234), checks only that one in its homomorphic ops
 * (:427-470, :472-513), declares generatePublicKey (ao-tfhe/eoc-tfhe-run.h:10) and leaves both it and the binding
 * (ao-tfhe/eoc-tfhe-bindings.c:51-57) empty; every op takes a base64PublicKey argument the bindings never fill
 * (:63-110).  Here the pair is real:
 *   client:  generateGateKey / generateSecretKey / importSecretKey, then exportCloudKey (= generatePublicKey)
 *   server:  importCloudKey -> a cloud-key-ONLY context: gate*, constantBit, addCiphertexts / subtractCiphertexts,
 *            eoc_global_gate_batch(_submit), eoc_global_circuit_run, eoc_global_params work; encryptBit, decryptBit,
 *            encryptInteger, decryptInteger, the ASCII-string calls, eoc_global_encrypt_bits / _decrypt_bits and
 *            exportSecretKey return NULL / -1 / EOC_ERR_NO_KEY with "Secret key not initialized..." on stderr.
 * One key per process (eoc-tfhe-run.cpp:245-249): importing into a context that has a key fails; resetGateKey clears.
 * The EOCCK1 blob is 83 MB (Set A) / 145 MB (Set B): next to the reference-style base64 string form there are a
 * file form and a raw-buffer form.
 * ---------------------------------------------------------------------------------------------- */
const char *exportCloudKey(void);                    /* base64(EOCCK1) of the global key, NULL without one */
int importCloudKey(const char *base64CloudKey);      /* 0, or -1 (malformed / a secret-key blob / a key already exists) */
int exportCloudKeyToFile(const char *path);          /* raw EOCCK1 bytes; 0 or -1 */
int importCloudKeyFromFile(const char *path);        /* 0 or -1 */
size_t eoc_global_cloud_key_export(void *buf, size_t cap); /* bytes needed (0 without a key); fills buf when cap suffices */
int eoc_global_import_cloud_key_blob(const void *buf, size_t len);
int eoc_global_key_mode(void);                       /* 0 no key, 1 secret + cloud key, 2 cloud key only (server) */

/* ------------------------------------------------------------------------------------------------
 * compact public-key encryption: a third party encrypts with an 8 KiB public key into compact lists, a
 * server turns them into ordinary gate / LUT inputs with the cloud key it already holds.
 *   public key  pk = (A, B) in Z_2^32[X]/(X^N + 1), B = A s' + e: one bootstrapping-key row with message 0 under the TLWE
 *               key s' -- A[j] = torus(j), e[j] = gaussian(N + 2j, 0, bk_stdev) from the secret key's own source (seeded
 *               or ChaCha20) under stream tag 6 (PublicKey), index 0.  The same secret key always gives the same public key.
 *               Blob "EOCPK1\0\0" | params (as EOCSK1 / EOCCK1) | A int32[N] | B int32[N], little-endian: 8 236 bytes.
 *   list        list L of a call holds messages L N ... L N + N - 1 as one TLWE sample (c0, c1), [2][N] int32, c0 first:
 *               u[i] = bit(i) (binary), e1[j] = gaussian(N + 2j), e2[j] = gaussian(3N + 2j), both bk_stdev, from the
 *               encryptor's stream tag 7 (CompactEnc), index first_list + L;  c0 = u A + e1,  c1 = u B + e2 + M.
 *               Slots past `count` in the last list encrypt 0.  8 KiB carry N = 1024 messages: 8 bytes per message against
 *               4 (n + 1) for an LWE sample (250 x smaller on Set A, 315 x on Set B).  `lists` has room for ceil(count / N).
 *   messages    bits at +-2^29 (eoc_encrypt_bits' encoding), integers m in Z_p at m 2^32 / (2p), p in {2, 4, 8}
 *               (eoc_encrypt_ints' encoding).
 *   expansion   eoc_compact_expand_device / eoc_compact_expand: slot j's extracted sample has phase M_j + u e + e2 - e1 s'
 *               under s' (sigma ~2e-7 on Set A, ~1e-6 on Set B: eoc_tfhe_amd/noise.compact_var); after the key switch the
 *               error is the key switch's (sigma ~0.0019 / ~0.0024), below a gate output's (~0.0042 / ~0.0035), so every
 *               decision margin stated for gate outputs holds for expanded inputs.
 *   randomness  eoc_pk_encrypt_bits / _ints with enc_seed: REPRODUCIBLE / TEST mode (splitmix64 streams, shared with the
 *               oracle) -- NOT secure, as for eoc_encrypt_bits.  The _keyed forms: ChaCha20 streams under the caller's
 *               256-bit enc_key.  NEVER encrypt two lists under one (key, list index) pair: they share u, e1 and e2, so
 *               c1 - c1' = M - M' and the difference of the messages is in the clear.  The Python wrappers draw a fresh
 *               key from the OS per call (and fail if none is available), so they cannot repeat a pair.
 *   security    the public key and every list are ring-LWE samples in the bootstrapping key's ring (N = 1024, modulus 2^32)
 *               with its noise (bk_stdev) and a binary secret (s' for the key, u for a list): they rest on the assumption
 *               the published bootstrapping key already rests on, and nothing beyond it is claimed.
 * Client side, CPU only, multithreaded over lists (eoc_host_threads).  EOC_ERR_ARG, with nothing written, for a null pointer,
 * a blob that is not a whole EOCPK1 blob (wrong magic, truncated, an EOCCK1 or EOCSK* blob), p outside {2, 4, 8} or a
 * value >= p; count 0 is a no-op. */
size_t eoc_public_key_blob_bytes(const eoc_params *p);                            /* 8 236 for both default sets */
int eoc_public_key_export(const eoc_secret_key *sk, void *buf, size_t cap);       /* EOC_ERR_ARG when cap is too small */
int eoc_public_key_blob_params(const void *buf, size_t len, eoc_params *p);       /* a whole EOCPK1 blob, else EOC_ERR_ARG */
int eoc_pk_encrypt_bits(const void *pk, size_t pk_len, uint64_t enc_seed, uint64_t first_list, const uint8_t *bits,
                        size_t count, int32_t *lists);
int eoc_pk_encrypt_bits_keyed(const void *pk, size_t pk_len, const uint8_t enc_key[32], uint64_t first_list,
                              const uint8_t *bits, size_t count, int32_t *lists);
int eoc_pk_encrypt_ints(const void *pk, size_t pk_len, uint64_t enc_seed, uint64_t first_list, int p, const uint8_t *values,
                        size_t count, int32_t *lists);
int eoc_pk_encrypt_ints_keyed(const void *pk, size_t pk_len, const uint8_t enc_key[32], uint64_t first_list, int p,
                              const uint8_t *values, size_t count, int32_t *lists);
/* lists [ceil(count / N)][2][N] -> out [count][n+1] on the global context (host buffers, synchronous): samples are cut into
 * eoc_shard_range blocks, one per engine, and each engine receives only the lists its block touches.  The engines come up
 * behind the global key on first use; the cloud key alone suffices (key mode 2).  EOC_ERR_ARG for a null pointer. */
int eoc_compact_expand(const int32_t *lists, size_t count, int32_t *out);
/* EOCPK1 blob of the global secret key (key mode 1): bytes needed, 0 without a secret key; fills buf when cap suffices */
size_t eoc_global_public_key_export(void *buf, size_t cap);

/* ------------------------------------------------------------------------------------------------
 * leveled operations: TGSW selectors, CMux, and reading entry idx of a table when idx is encrypted.
 *   selector    a TGSW sample of one bit in torus form, [2l][2][N] int32: the shape and convention of one bk[i] block --
 *               2l TLWE encryptions of 0 under s' at bk_stdev, mask first; for bit 1, row (q, p) carries 2^(32 - p Bgbit) on
 *               the constant coefficient of polynomial q.  32 KiB (Set A) / 48 KiB (Set B).  Row `row` of selector s uses
 *               stream tag 8 (TgswEnc), index (first_idx + s) 2l + row, with make_bk's counters (mask word j at j, Gaussian
 *               j at N + 2j).  eoc_tgsw_encrypt_bits is the REPRODUCIBLE / TEST mode and is refused (EOC_ERR_STATE) for a
 *               secure-mode key; the _keyed form draws ChaCha20 streams under the caller's 256-bit key.  NEVER encrypt two
 *               selectors under one (key, index) pair: they share masks and noise, and their difference is the gadget of
 *               the bit difference in the clear.  The Python wrapper of the secure path draws a fresh key per call.
 *   security    selectors are ring-LWE samples of the bootstrapping key's ring at its noise: the assumption the published
 *               bootstrapping key already rests on.
 *   table       TLWE samples [2^d][2][N] holding N slots each: compact lists (eoc_pk_encrypt_*), or public data as trivial
 *               samples (eoc_table_trivial: c0 = 0, c1 = the messages; list L holds messages L N ... L N + N - 1).
 *   device form eoc_tgsw_to_fft_device: the key-load transform; a converted selector is laid out like one row block of the
 *               bootstrapping key's FFT image, [2l][2][512] complex f64 scaled by 2^-9 (eoc_tgsw_fft_bytes: 64 / 96 KiB).
 *   CMux        eoc_cmux_device: out[i] = in0[i] + C[i] (x) (in1[i] - in0[i]) -- in1 if the bit is 1, in0 otherwise, plus
 *               noise.cmux_var.  Needs no key.  `out` may not overlap the inputs.
 *   read        eoc_table_read_device: W = 2^log2_width consecutive slots form an entry, the table has 2^(d + r) entries,
 *               d = log2_lists in [0, 12], r = 10 - log2_width in [0, 10].  Index bits LSB first: bits 0 .. r-1 pick the entry
 *               inside a list (slot offset W (idx mod 2^r)), bits r .. r+d-1 the list; d_sel_fft is [queries][r + d] converted
 *               selectors in that order.  First the CMux tree over the lists (level v under bit r + v), then r rotations by
 *               X^(-W 2^i) under bit i (ascending), then slots 0 .. W-1 are extracted and key-switched: d_out is
 *               [queries][W][n+1], ordinary gate / LUT inputs whose error is below a gate output's (noise.table_read_var).
 *               Only the key switch needs the cloud key (EOC_ERR_NO_KEY without one).  Workspace: two buffers of
 *               queries 2^(d-1) and queries 2^(d-2) TLWE samples, grown by eoc_engine_reserve's rule (EOC_ERR_STATE under
 *               capture); queries are sliced so that both stay within 256 MiB (EOC_TFHE_TABLE_WS_BYTES at engine creation
 *               changes the budget and no result; a budget below one query's need is EOC_ERR_ARG) and a slice extracts at
 *               most 2^20 samples.  Stats: keyswitches += queries W; eoc_engine_cmux_launches counts the k_cmux launches
 *               (r + d per slice); eoc_engine_kernel_times books them under the blind rotation.
 * EOC_ERR_ARG for a null pointer, log2_lists outside [0, 12] or log2_width outside [0, 10]; count / queries 0 is a no-op. */
size_t eoc_tgsw_len(const eoc_params *p);      /* int32 count of one selector: 2l * 2 * N */
int eoc_tgsw_encrypt_bits(const eoc_secret_key *sk, uint64_t enc_seed, uint64_t first_idx, const uint8_t *bits, size_t count,
                          int32_t *out);
int eoc_tgsw_encrypt_bits_keyed(const eoc_secret_key *sk, const uint8_t enc_key[32], uint64_t first_idx, const uint8_t *bits,
                                size_t count, int32_t *out);
/* on the global secret key, with its encryption randomness (eoc_global_encrypt_bits); EOC_ERR_NO_KEY on a cloud-key-only context */
int eoc_global_tgsw_encrypt_bits(const uint8_t *bits, size_t count, int32_t *out);
int eoc_table_trivial(const int32_t *messages, size_t count, int32_t *lists); /* lists [ceil(count / N)][2][N] */
size_t eoc_tgsw_fft_bytes(const eoc_params *p);   /* 2l * 2 * 512 * 16 = eoc_bkfft_bytes(p) / n */
int eoc_tgsw_to_fft_device(eoc_engine *e, const int32_t *d_tgsw, size_t count, void *d_fft, void *hip_stream);
int eoc_cmux_device(eoc_engine *e, const void *d_sel_fft, const int32_t *d_in0, const int32_t *d_in1, int32_t *d_out,
                    size_t count, void *hip_stream);
int eoc_table_read_device(eoc_engine *e, const int32_t *d_table, int log2_lists, int log2_width, const void *d_sel_fft,
                          size_t queries, int32_t *d_out, void *hip_stream);
uint64_t eoc_engine_cmux_launches(eoc_engine *e);
/* the read on the global context (host buffers, synchronous): table [2^d][2][N], selectors in TORUS form [queries][r + d][2l][2][N],
 * out [queries][W][n+1].  Queries are cut into eoc_shard_range blocks, one per engine; every engine receives the whole table
 * and converts its own selectors.  The cloud key alone suffices (key mode 2). */
int eoc_table_read(const int32_t *table, int log2_lists, int log2_width, const int32_t *selectors, size_t queries, int32_t *out);

/* ------------------------------------------------------------------------------------------------
 * encrypted-index table updates: table[idx_q] += value_q under encrypted idx_q -- the read run backwards.
 *   demux       eoc_demux_device: E = C[i] (x) in[i]; out1[i] = E, out0[i] = in[i] - E word by word: in[i] goes to out1 where
 *               the bit is 1 and to out0 otherwise, the other child is an encryption of 0.  E is the CMux's external product
 *               (in0 = 0, in1 = in[i]) bit for bit.  accumulate = 0 stores (the outputs may not overlap the input),
 *               accumulate != 0 ADDS both children into out0 / out1 with integer atomics.  Needs no key.
 *   update      eoc_table_update_device: the table [2^d][2][N] is updated IN PLACE; d, W = 2^log2_width, r = 10 - log2_width and
 *               d_sel_fft [queries][r + d] are the read's, so one encrypted index serves a read and an update of the same
 *               entry.  d_vals is [queries][2][N] TLWE samples under s' whose slots 0 .. W-1 carry the entry's W messages and
 *               every other slot message 0 (a packed list of W samples, a public-key list, eoc_table_trivial); what the other
 *               slots carry is added to the neighbouring entries of the selected list.  Per query: r rotations by X^(W 2^i)
 *               under bit i ascending (k_cmux), then d demux stages, stage t under bit r + (d - 1 - t), parent j -> children
 *               2j (x - E) and 2j + 1 (E); the last stage adds its 2^d leaves into the table.  Every word is a wrapping
 *               integer sum: queries on one index, any slicing and any order give the same words.  d = r = 0 is a plain
 *               wrapping add and takes d_sel_fft = NULL.  Needs no key.  Workspace, budget, slicing and their error codes
 *               are the read's.  Stats: eoc_engine_demux_launches counts the k_demux launches (d per slice),
 *               eoc_engine_cmux_launches advances by r per slice; eoc_engine_kernel_times books all of them under the blind
 *               rotation.  Noise: noise.table_update_var / table_update_mean.
 * EOC_ERR_ARG for a null pointer or a shape outside the read's ranges; count / queries 0 is a no-op. */
int eoc_demux_device(eoc_engine *e, const void *d_sel_fft, const int32_t *d_in, int32_t *d_out0, int32_t *d_out1, size_t count,
                     int accumulate, void *hip_stream);
int eoc_table_update_device(eoc_engine *e, int32_t *d_table, int log2_lists, int log2_width, const void *d_sel_fft,
                            const int32_t *d_vals, size_t queries, void *hip_stream);
uint64_t eoc_engine_demux_launches(eoc_engine *e);
/* the update on the global context (host buffers, synchronous): table [2^d][2][N] updated in place, selectors in TORUS form
 * [queries][r + d][2l][2][N], values [queries][2][N].  Queries are cut into eoc_shard_range blocks; every engine accumulates its
 * block into a zeroed table of its own and the host adds those into `table` in wrapping arithmetic: any engine count gives the
 * single-engine words.  The cloud key alone suffices (key mode 2). */
int eoc_table_update(int32_t *table, int log2_lists, int log2_width, const int32_t *selectors, const int32_t *values,
                     size_t queries);

/* ------------------------------------------------------------------------------------------------
 * finite automata on encrypted bit strings: a PUBLIC deterministic (weighted) automaton run over a string of
 * TGSW-encrypted bits, one external product per state and input bit, no bootstrap.
 *   automaton   `states` states, trans HOST [states][4] int32 = {next0, w0, next1, w1}: the successor and the weight under input
 *               bit 0 / bit 1; successors in [0, states), weights in [0, 2N), states in [1, 4096].  starts HOST [n_starts] state
 *               ids, n_starts in [1, 4096].  Both are validated on the host before anything touches a device (EOC_ERR_ARG) and
 *               travel through the engine's descriptor ring: the calls stay asynchronous and can be captured.
 *   query       `steps` converted selectors (eoc_tgsw_to_fft_device); selector t holds input bit t, bit 0 is read FIRST by the
 *               automaton.  d_sel_fft is [queries][steps].
 *   final       d_final [states][2][N] TLWE samples under s': trivial (eoc_table_trivial) or encrypted lists.  An acceptor puts
 *               mu on slot 0 of the accepting states; a weighted automaton puts a public table in the slots.
 *   rule        V_steps = final;  V_t[q] = A + C_t (x) (B - A),  A = X^(-w0(q)) V_(t+1)[next0(q)],  B = X^(-w1(q)) V_(t+1)[next1(q)],
 *               t = steps - 1 .. 0; the result for start state s is V_0[s], whose slots 0 .. W-1 (W = 2^log2_width) are extracted
 *               and key-switched as a table read's: d_out [queries][n_starts][W][n+1].  Slot 0 holds final[end state] at slot
 *               (sum of the weights along the run), negacyclically.  steps = 0 extracts from d_final directly.
 *   step        eoc_automaton_step_device: one step for every state and query, the building block (eoc_cmux_device's
 *               counterpart): d_prev [states][2][N] per query, prev_query_stride TLWE samples between the queries' vectors (0:
 *               one vector shared by all queries; otherwise >= states), selector of query q at q sel_query_stride selectors,
 *               d_next [queries][states][2][N], which may not overlap d_prev.  Needs no key.
 *   run         eoc_automaton_run_device: `steps` launches per slice of queries (the last over the start states alone), then
 *               the extraction and the key switch (EOC_ERR_NO_KEY without a cloud key).  Workspace: two state vectors of
 *               queries max(states, n_starts) TLWE samples in the table read's buffers, grown by eoc_engine_reserve's rule
 *               (EOC_ERR_STATE under capture), held to the read's byte budget (EOC_TFHE_TABLE_WS_BYTES; a budget below one
 *               query's need is EOC_ERR_ARG); a slice extracts at most 2^20 samples.  Stats: keyswitches += queries n_starts W;
 *               eoc_engine_automaton_launches counts the k_automaton_step launches (steps per slice) and
 *               eoc_engine_cmux_launches does not move; eoc_engine_kernel_times books them under the blind rotation.
 *   noise       additive: noise.automaton_var / automaton_mean_bound / automaton_budget.
 *   security    the selectors are the table read's (above); the automaton, the start states and the string length are public.
 * EOC_ERR_ARG for a null pointer or a malformed automaton; queries 0 is a no-op. */
int eoc_automaton_step_device(eoc_engine *e, const int32_t *trans, size_t states, const int32_t *d_prev, size_t prev_query_stride,
                              const void *d_sel_fft, size_t sel_query_stride, int32_t *d_next, size_t queries, void *hip_stream);
int eoc_automaton_run_device(eoc_engine *e, const int32_t *trans, size_t states, const int32_t *d_final, const void *d_sel_fft,
                             size_t steps, const int32_t *starts, size_t n_starts, int log2_width, int32_t *d_out, size_t queries,
                             void *hip_stream);
uint64_t eoc_engine_automaton_launches(eoc_engine *e);
/* the run on the global context (host buffers, synchronous): final_vec [states][2][N], selectors in TORUS form
 * [queries][steps][2l][2][N] (NULL at steps = 0), out [queries][n_starts][W][n+1].  The automaton is validated before a key or a
 * device is looked for.  Queries are cut into eoc_shard_range blocks, one per engine; every engine receives the final vector and
 * converts its own selectors.  The cloud key alone suffices (key mode 2). */
int eoc_automaton_run(const int32_t *trans, size_t states, const int32_t *final_vec, const int32_t *selectors, size_t steps,
                      const int32_t *starts, size_t n_starts, int log2_width, int32_t *out, size_t queries);

/* ------------------------------------------------------------------------------------------------
 * rounding mode of the leveled calls: an opt-in gadget decomposition that rounds where the oracle's truncates.
 *   rule        with h = 2^(31 - l Bgbit) where l Bgbit < 32 and h = 0 otherwise, every external product C (x) D of the calls
 *               below becomes C (x) (D + h), h added to every coefficient word of both polynomials, wrapping: the CMux is
 *               out = in0 + C (x) ((X^rot in1 - in0) + h), the demux E = C (x) (in + h), the automaton step likewise.  The part
 *               of a word the gadget drops then lies in [-q/2, q/2), q = 2^(32 - l Bgbit), and not in [0, q): the mean it
 *               leaves in every product whose bit is 1 falls from -(q/2) (J (1 - s')) to -2^-33 (J (1 - s')) per slot; the
 *               variance (noise.cmux_var) is unchanged.  Long leveled chains -- automata, tables updated many times -- are
 *               bound by that mean in the default mode (noise.automaton_budget, noise.table_update_budget).
 *   mode        off (0) at engine creation: every word is the oracle's.  eoc_engine_set_leveled_rounding(e, 1) makes
 *               eoc_cmux_device, eoc_table_read_device, eoc_demux_device, eoc_table_update_device,
 *               eoc_automaton_step_device and eoc_automaton_run_device launch the rounding twins of their kernels (k_rcmux,
 *               k_rdemux, k_rstep; the launch counters are shared with the default kernels).  Nothing else is governed by it:
 *               no blind rotation (the encrypted-seed one included), no key switch, no packing call.  Where l Bgbit = 32 the
 *               mode changes no word.  A sample produced in one mode is an ordinary input of the other.
 *   capture     a captured graph replays the mode it was captured under.  While a capture that already holds one of the
 *               calls above is open on the engine, the setter returns EOC_ERR_STATE and changes nothing.
 *   global      eoc_global_set_leveled_rounding(on) sets every engine of the global context and is remembered for engines
 *               the context creates later (it may be called before eoc_gpu_init); eoc_table_read, eoc_table_update and
 *               eoc_automaton_run follow it.  Any engine count gives the single-engine words of the same mode.
 * EOC_ERR_ARG for a null engine or an `on` other than 0 and 1. */
int eoc_engine_set_leveled_rounding(eoc_engine *e, int on);
int eoc_engine_leveled_rounding(const eoc_engine *e);   /* 0 or 1; 0 for a null engine */
int eoc_global_set_leveled_rounding(int on);

/* ------------------------------------------------------------------------------------------------
 * packing key switch: LWE samples under the LWE key s (gate or LUT outputs) -> compact TLWE lists under s',
 * the layout of eoc_pk_encrypt_*, eoc_table_trivial and the table of eoc_table_read_device.  1 024 results leave in 8 KiB
 * instead of 2 MB (Set A) / 2.5 MB (Set B), and a value the server computed can become a table.
 *   packing key Row (m, j), m < n, j = 1 .. 4: a TLWE encryption under s' at bk_stdev of the constant polynomial
 *               s_m 2^(32 - 4j) -- the mask and noise of one TGSW row with bit 0 (mask word k at counter k, Gaussian k at
 *               N + 2k) from the secret key's own source under stream tag 9 (PackKsk), index 4 m + (j - 1), plus
 *               2^(32 - 4j) on b[0] when s_m = 1.  The same secret key always gives the same packing key.  The decomposition
 *               is FIXED at t = 4, basebit = 4 (EOC_PACK_T, EOC_PACK_BASEBIT: 16 bits of precision).
 *               Blob "EOCPKS1\0" | params (as EOCCK1) | t, basebit (2 x i32) | rows int32[n][4][2][N], little-endian:
 *               16.4 MB (Set A) / 20.6 MB (Set B).  A blob of its own: EOCCK1 and the cloud-key calls are unchanged.
 *   operation   sample i goes to slot i mod N of list i / N; slots past `count` in the last list behave as samples (0, 0).
 *               Per list, in wrapping 32-bit arithmetic: A_m(X) = sum_i a_{i,m} X^i, B(X) = sum_i b_i X^i,
 *               out = (0, B) - sum_m sum_j D_{m,j}(X) Row(m, j), with digit d_j = ((x >> (32 - 4j)) & 15) - 8 of
 *               x = a + 2^15 + sum_p 8 2^(32 - 4p): a ROUNDING decomposition (no mean is left).  The rows of 16 consecutive
 *               key indices (a chunk; the last one is short) are accumulated in the spectral domain, m ascending then j
 *               ascending, first term a product and every later one the two-FMA chain, inverse-transformed and converted
 *               ONCE per chunk (|.| <= 2^50: exact conversion on every parameter set) and subtracted as int32; chunks
 *               combine by integer addition, in any order.  The chunk is part of the format: eoc_pack_device equals the
 *               CPU reference tests/c/pack_ref.c byte for byte.
 *   noise       noise.pack_var: sigma ~9e-5 (Set A) / ~3e-4 (Set B) for a full list, far below a gate output's; mean 0.
 *   security    the rows are ring-LWE samples of the bootstrapping key's ring under s' that encrypt bits of s: the
 *               circular-security assumption the published key-switch and bootstrapping keys already make.
 *   engine      eoc_engine_set_packing_key parses the blob, checks its parameters against the engine's, uploads and converts
 *               the rows (the key-load transform, [n][4][2][512] complex f64 scaled by 2^-9: 32.8 / 41.3 MB, owned by the
 *               engine) and replaces an earlier image.  eoc_pack_device: d_in DEVICE [count][n+1], d_lists DEVICE
 *               [ceil(count / N)][2][N]; EOC_ERR_NO_KEY without a packing key, count 0 is a no-op.  Workspace: the mask
 *               columns [lists][n][N] int32, grown by eoc_engine_reserve's rule (EOC_ERR_STATE under capture); lists are
 *               sliced so that it stays within 256 MiB (EOC_TFHE_PACK_WS_BYTES at engine creation changes the budget and no
 *               result; a budget below one list's need is EOC_ERR_ARG).  No descriptor slot is used.  Stats:
 *               eoc_engine_pack_launches (one per slice), eoc_engine_packed_samples; eoc_engine_kernel_times books the
 *               kernels under the key switch.  Asynchronous on hip_stream.
 * Malformed, truncated or mismatched blobs (wrong magic, t or basebit other than 4, another parameter set than the
 * engine's / the context's) are EOC_ERR_ARG. */
#define EOC_PACK_T 4
#define EOC_PACK_BASEBIT 4
size_t eoc_packing_key_blob_bytes(const eoc_params *p);
int eoc_packing_key_export(const eoc_secret_key *sk, void *buf, size_t cap);       /* EOC_ERR_ARG when cap is too small */
int eoc_packing_key_blob_params(const void *buf, size_t len, eoc_params *p);       /* a whole EOCPKS1 blob, else EOC_ERR_ARG */
int eoc_engine_set_packing_key(eoc_engine *e, const void *blob, size_t len);
int eoc_pack_device(eoc_engine *e, const int32_t *d_in, size_t count, int32_t *d_lists, void *hip_stream);
uint64_t eoc_engine_pack_launches(eoc_engine *e);
uint64_t eoc_engine_packed_samples(eoc_engine *e);
/* client side: the phases c1 - c0 s' of every slot, phases [n_lists][N]; the first `count` slots of lists
 * [ceil(count / N)][2][N] as bits (phase > 0, eoc_decrypt_bits' rule) or as integers of Z_p (eoc_decrypt_ints' rule) */
int eoc_list_phases(const eoc_secret_key *sk, const int32_t *lists, size_t n_lists, int32_t *phases);
int eoc_decrypt_list_bits(const eoc_secret_key *sk, const int32_t *lists, size_t count, uint8_t *bits);
int eoc_decrypt_list_ints(const eoc_secret_key *sk, int p, const int32_t *lists, size_t count, uint8_t *values);
/* on the global context.  The three client calls and the export need the secret key (EOC_ERR_NO_KEY / 0 in key mode 2);
 * eoc_global_import_packing_key_blob gives every engine of the context the packing key and works behind a cloud key alone
 * (key mode 2); eoc_pack (host buffers, synchronous) cuts WHOLE lists into eoc_shard_range blocks, one per engine. */
int eoc_global_list_phases(const int32_t *lists, size_t n_lists, int32_t *phases);
int eoc_global_decrypt_list_bits(const int32_t *lists, size_t count, uint8_t *bits);
int eoc_global_decrypt_list_ints(int p, const int32_t *lists, size_t count, uint8_t *values);
size_t eoc_global_packing_key_export(void *buf, size_t cap); /* bytes needed (0 without a secret key); fills buf when cap suffices */
int eoc_global_import_packing_key_blob(const void *buf, size_t len);
int eoc_pack(const int32_t *cts, size_t count, int32_t *lists);

/* ---- two-input table lookups: blind rotation from an encrypted polynomial --------------------------------
 * F(x, y) on Z_p x Z_p, p in {2, 4, 8}, by the tree method: level 1 bootstraps x against the p public tables x -> F(x, j)
 * (T = max(n_tables, 1) tables per blind rotation), the packing key switch lays the p results v_0 .. v_(p-1) of a row out as
 * ONE TLWE test polynomial by eoc_lut_test_polynomial's rule, and level 2 blind-rotates that ENCRYPTED polynomial by y,
 * extracts and key-switches: v_y = F(x, y), with refreshed noise (noise.lut2_var).
 *   eoc_lut2_test_polynomials   host: table [p][p] of Torus32 output values, table[x p + y]; writes tv [p / T][N], polynomial
 *               g holding the tables y = g T .. g T + T - 1 as eoc_lut_many_test_polynomial (T > 1) or
 *               eoc_lut_test_polynomial (T = 1) lays them out.  EOC_ERR_ARG for a null pointer, p outside {2, 4, 8}, T outside
 *               {1, 2, 4, 8}, T not dividing p, or p T > 16 at T > 1.
 *   eoc_lut_enc_batch_device    level 2 alone: d_lists DEVICE TLWE samples [..][2][N] (c0 first: eoc_pack_device,
 *               eoc_pk_encrypt_*, eoc_table_trivial), d_in DEVICE [count][n+1], d_out DEVICE [n_groups][count][n+1].  Job
 *               (g, s) starts from ACC = X^(-barb_s) (c0, c1) of list g (per_row == 0) or list g x count + s (per_row != 0)
 *               and is rotated by input row s: k_prepare, ONE blind rotation of the k_br_enc / k_br_enc_wide family through
 *               the gate levels' launch policy, the key switch.  Rows are sliced by eoc_lut_batch_device's 2^20 rule; the
 *               cloud key alone suffices.  EOC_TFHE_BR_TABLES_LDS=1 does not apply: the family has no earlier-form twin.
 *               Stats: bootstraps and keyswitches += n_groups x count.  EOC_ERR_ARG for a null pointer or n_groups outside
 *               [1, 32 768].
 *   eoc_tv_pack_device          d_vals DEVICE [n_funcs][p][count][n+1] (eoc_lut_batch_device's / eoc_lut_many_batch_device's
 *               output order), d_lists DEVICE [n_funcs][count][2][N]: list (f, s) = the packing key switch of the N-row batch
 *               in which coefficient k < N - N / (2p) holds sample v_j, j = (k p + N / 2) / N, and the last N / (2p)
 *               coefficients hold -v_0 (word-wise) -- word for word what eoc_pack_device gives for that batch, which is never
 *               materialised.  EOC_ERR_NO_KEY without a packing key; lists are sliced by eoc_pack_device's column budget.
 *               eoc_engine_pack_launches counts one per slice, eoc_engine_packed_samples the n_funcs x count x p samples READ.
 *   eoc_lut2_batch_device       d_tv0 DEVICE [n_funcs][p / T][N] (eoc_lut2_test_polynomials per function), d_x, d_y DEVICE
 *               [count][n+1] at message space p, d_out DEVICE [n_funcs][count][n+1].  Rows are sliced so that the level-1
 *               outputs (at most 2^20) and the lists (8 KiB each) of a slice fit 256 MiB; that buffer grows by
 *               eoc_engine_reserve's rule (EOC_ERR_STATE under capture: run one call of the captured shape first).  Needs the
 *               cloud key and the packing key (EOC_ERR_NO_KEY).  Stats: bootstraps += n_funcs x count x (p / T + 1),
 *               keyswitches += n_funcs x count x (p + 1).  EOC_ERR_ARG as eoc_lut2_test_polynomials, for n_tables < 0 and for
 *               n_funcs x p outside [1, 32 768].  count == 0 is a no-op.
 *   eoc_lut2_batch              global context, host buffers, synchronous: tables [n_funcs][p][p] of Torus32 output values,
 *               x, y [count][n+1], out [n_funcs][count][n+1]; rows are cut into eoc_shard_range blocks, one per engine.  Works
 *               in key mode 2 once eoc_global_import_packing_key_blob has run; EOC_ERR_NO_KEY otherwise. */
int eoc_lut2_test_polynomials(int p, int n_tables, const int32_t *table, int32_t *tv);
int eoc_lut_enc_batch_device(eoc_engine *e, const int32_t *d_lists, size_t n_groups, int per_row, const int32_t *d_in,
                             int32_t *d_out, size_t count, void *hip_stream);
int eoc_tv_pack_device(eoc_engine *e, int p, const int32_t *d_vals, size_t n_funcs, size_t count, int32_t *d_lists,
                       void *hip_stream);
int eoc_lut2_batch_device(eoc_engine *e, int p, int n_tables, const int32_t *d_tv0, size_t n_funcs, const int32_t *d_x,
                          const int32_t *d_y, int32_t *d_out, size_t count, void *hip_stream);
int eoc_lut2_batch(int p, int n_tables, const int32_t *tables, size_t n_funcs, const int32_t *x, const int32_t *y, int32_t *out,
                   size_t count);

/* ---- multi-digit table lookups: deeper trees on an exact matrix-core pack ----------------------------------
 * F on Z_p^d, p in {2, 4, 8}, 2 <= d <= 4, p^(d-1) <= 64: level 1 bootstraps x_1 against the p^(d-1) public tables
 * x_1 -> F(x_1, j_2, .., j_d); for every further digit k the EXACT pack puts the p values that differ only in j_k into one
 * encrypted test polynomial and a blind rotation by x_k (eoc_lut_enc_batch_device's family) selects one of them.
 *   eoc_tv_pack_exact_device    arguments, layouts and checks of eoc_tv_pack_device.  Per list, with the values v_0 .. v_(p-1),
 *               h = N / (2p), w = N / p, in wrapping 32-bit integers: samples u_s = v_s (s < p), u_p = v_0 negated word by word;
 *               S_s = (0, b_s X^0) - sum_m sum_j d_(s,m,j) Row(m, j) with the signed base-16 digits of eoc_pack_device (offset
 *               2^15 + sum 8 2^(32 - 4j), values in [-8, 8)) and Row the int32 rows of the EOCPKS1 blob; list = sum_s Win_s(X) S_s
 *               as negacyclic products, Win_0 = X^0 + .. + X^(h-1), Win_s = X^(s w - h) + .. + X^(s w + h - 1) (0 < s < p),
 *               Win_p = X^(N-h) + .. + X^(N-1).  This is the EXACT value of the rule eoc_tv_pack_device evaluates within the
 *               rounding of its transforms (at most 8 LSB per chunk of 16 key indices); same noise (noise.pack_var at N filled
 *               slots).  The constant-slot samples S ((p + 1) x 8 KiB per list) live in a scratch buffer under
 *               eoc_engine_reserve's rule (EOC_ERR_STATE if it would grow under capture), lists sliced by
 *               EOC_TFHE_PACK_WS_BYTES (no word depends on it; below one list's need: EOC_ERR_ARG).  Stats as
 *               eoc_tv_pack_device: one pack launch per slice, packed samples += n_funcs x count x p.  count == 0 is a no-op.
 *   eoc_lut_tree_test_polynomials   host: table [p^d] of Torus32 output values, table[(..(x_1 p + x_2) p + ..) p + x_d] (at
 *               d = 2: eoc_lut2_test_polynomials' table); writes tv [p^(d-1) / T][N].  Level-1 table J = j_2 + p j_3 + p^2 j_4
 *               (j_2 FASTEST, j_d slowest) is x_1 -> F(x_1, j_2, .., j_d); polynomial g holds the tables J = g T .. g T + T - 1.
 *               EOC_ERR_ARG for a null pointer, p outside {2, 4, 8}, d outside [2, 4], p^(d-1) > 64, T outside {1, 2, 4, 8}, T
 *               not dividing p, or p T > 16 at T > 1.
 *   eoc_lut_tree_batch_device   d_tv0 DEVICE [n_funcs][p^(d-1) / T][N], d_digits DEVICE [d][count][n+1] (x_1 first) at message
 *               space p, d_out DEVICE [n_funcs][count][n+1].  Rows are sliced so that a slice's level-1 outputs (at most 2^20)
 *               and first-pack lists fit 256 MiB; that buffer grows by eoc_engine_reserve's rule.  Needs the cloud key and the
 *               packing key (EOC_ERR_NO_KEY).  Stats: bootstraps += n_funcs x count x (p^(d-1) / T + sum_(k=2..d) p^(d-k)),
 *               keyswitches += n_funcs x count x sum_(k=1..d) p^(d-k).  EOC_ERR_ARG as eoc_lut_tree_test_polynomials, for
 *               n_tables < 0 and for n_funcs x p^(d-1) outside [1, 32 768].  count == 0 is a no-op.  Nothing is refused on
 *               noise grounds: noise.lut_tree_var / lut_tree_margin_sigma give the budget.
 *   eoc_lut_tree_batch          global context, host buffers, synchronous: tables [n_funcs][p^d], digits [d][count][n+1], out
 *               [n_funcs][count][n+1]; rows are cut into eoc_shard_range blocks, one per engine.  Works in key mode 2 once
 *               eoc_global_import_packing_key_blob has run; EOC_ERR_NO_KEY otherwise. */
int eoc_tv_pack_exact_device(eoc_engine *e, int p, const int32_t *d_vals, size_t n_funcs, size_t count, int32_t *d_lists,
                             void *hip_stream);
int eoc_lut_tree_test_polynomials(int p, int d, int n_tables, const int32_t *table, int32_t *tv);
int eoc_lut_tree_batch_device(eoc_engine *e, int p, int d, int n_tables, const int32_t *d_tv0, size_t n_funcs,
                              const int32_t *d_digits, int32_t *d_out, size_t count, void *hip_stream);
int eoc_lut_tree_batch(int p, int d, int n_tables, const int32_t *tables, size_t n_funcs, const int32_t *digits, int32_t *out,
                       size_t count);

/* ---- seeded ciphertexts, selectors and cloud key: masks expanded on the GPU ---------------------------------
 * Every LWE sample, TGSW row and key row is a uniform mask plus a body.  In the seeded forms the holder of the secret key
 * sends the bodies and a PUBLIC 32-byte seed; the receiver regenerates the masks.  No key, no key switch, no extra noise.
 *   mask streams the generator of the secure mode (ChaCha20, RFC 8439 block function) with the seed in the master key's
 *               place: stream (seed, tag, idx) has the sub-key = first half of block ChaCha20(seed, counter tag << 32, nonce
 *               idx); its word j is the HIGH half of the j-th 64-bit word of the blocks ChaCha20(sub-key, counter j / 8,
 *               nonce 0) -- a block yields 8 mask words.  Tags: 10 LWE samples (idx = first_idx + s), 11 bootstrapping-key rows
 *               (idx = row), 12 key-switch-key rows (idx = row), 13 selector rows (idx = (first_idx + s) 2l + row), 14 the
 *               seed of a cloud key.  Masks are ChaCha20 also for test-mode keys.
 *   noise       from the secret side, under the same tag and index and the unseeded code's counters: stream (enc_key, tag,
 *               idx) for samples and selectors, stream (key's source, tag, row) for key rows.
 *   LWE         sample s: a[m] = word m of stream (seed, 10, first_idx + s), b = gaussian(mu, ks_stdev) + <a, s>.  The wire
 *               form is the seed once per batch and 4 bytes per sample (2 004 bytes unseeded on Set A).
 *   selector    row (q, p) of selector s: a = the stream's N words, b = e + s' a - [q = 0] bit g_p s'(X) + [q = 1] bit g_p,
 *               g_p = 2^(32 - p Bgbit): eoc_tgsw_encrypt_bits' row computed on a - [q = 0] bit g_p (its gadget on a[0] depends
 *               on the bit and cannot come from a seed).  Same phase, same distribution; the expanded (a, b) is an ordinary
 *               row.  Bodies [count][2l][N]: half of a selector.
 *   cloud key   blob "EOCCKS1\0" | params (as EOCCK1) | seed[32] | BK bodies int32[n][2l][N] | KSK bodies
 *               int32[N t (base - 1)], little-endian: 8.3 MB (Set A) / 15.6 MB (Set B) against 65.6 / 93.0 MB of EOCCK1.
 *               It is a FRESH, INDEPENDENT encryption, not the EOCCK1 key with its masks swapped: the noise of its rows comes
 *               from streams (key's source, 11 / 12, row), never from the streams of eoc_sk_bk / eoc_sk_ksk, and its seed is
 *               32 bytes of the key's own source under tag 14 -- the export is deterministic: the same secret key always
 *               gives the same bytes.  EOCCK1, eoc_cloud_key_export and the arrays of a secret key are unchanged.
 * SECURITY, two rules.  (1) A (seed, tag, idx) triple must NEVER mask two different encryptions under one key: b1 - b2 would
 * be the message difference in the clear.  eoc_seeded_encrypt_bits / _ints and eoc_tgsw_seeded_encrypt_bits draw the mask
 * seed AND a noise key fresh from the OS per call, return the seed and take no first_idx (EOC_ERR_STATE without an entropy
 * source).  The _keyed forms take both keys and first_idx explicitly and are TEST-ONLY: the caller answers for never
 * repeating a triple and for an enc_key that is secret and unrelated to the seed.  (2) Two encryptions of one key under
 * different masks must not share their noise: b - b' = s (a - a') is linear algebra for the key.  Hence the independent noise
 * streams and the deterministic export above.
 * Client side and host twins (CPU, multithreaded; EOC_ERR_ARG for a null pointer, p outside {2, 4, 8} or a value >= p):
 *   eoc_seeded_expand_host       bodies[count] -> out[count][n+1]: what eoc_seeded_expand_device computes, word for word
 *   eoc_tgsw_seeded_expand_host  bodies[count][2l][N] -> out[count][2l][2][N], eoc_tgsw_encrypt_bits' layout
 *   eoc_seeded_cloud_key_expand  blob -> bk (eoc_bk_len words), ksk (eoc_ksk_len words): what eoc_engine_load_cloud_key and
 *                                the oracle accept.  A blob that is not a whole EOCCKS1 blob (wrong magic, wrong length,
 *                                invalid parameters) is EOC_ERR_ARG here and in every call that takes one.
 * Engine (k_seed_masks; eoc_engine_seed_launches counts its launches, eoc_engine_kernel_times books it under prepare):
 *   eoc_seeded_expand_device     d_bodies DEVICE [count], d_out DEVICE [count][n+1]; needs no key; asynchronous on hip_stream;
 *                                count 0 is a no-op; EOC_ERR_ARG when d_out overlaps d_bodies.  No workspace is used.
 *   eoc_tgsw_seeded_to_fft_device  d_bodies DEVICE [count][2l][N] (16-byte aligned) -> d_fft as eoc_tgsw_to_fft_device gives
 *                                for the host-expanded selectors, byte for byte.  The expanded torus form goes through a
 *                                staging buffer of at most 64 MiB that grows by eoc_engine_reserve's rule (EOC_ERR_STATE
 *                                under capture: run one call of the captured shape first).
 *   eoc_engine_load_seeded_cloud_key  uploads the bodies, expands on the device, transforms, installs the key-switch limbs:
 *                                the images are byte-identical to eoc_engine_load_cloud_key's on the host-expanded arrays.
 *                                Synchronous.  EOC_ERR_ARG when the blob's parameters are not the engine's.
 *   eoc_dbg_chacha20_blocks_device  d_out DEVICE [n_blocks][16] words: block i = ChaCha20(key, counter + i, nonce) in the
 *                                original layout (64-bit counter, 64-bit nonce), the kernels' block function.
 * Global context: eoc_seeded_expand (host buffers, synchronous) cuts the samples into eoc_shard_range blocks, one per engine;
 * eoc_global_import_seeded_cloud_key_blob installs a cloud-key-only context (key mode 2) whose engines each expand their own
 * copy of the key (no broadcast); eoc_global_cloud_key_export then returns the EOCCK1 blob of the host-expanded arrays. */
int eoc_seeded_encrypt_bits(const eoc_secret_key *sk, const uint8_t *bits, size_t count, uint8_t seed_out[32], int32_t *bodies);
int eoc_seeded_encrypt_ints(const eoc_secret_key *sk, int p, const uint8_t *values, size_t count, uint8_t seed_out[32],
                            int32_t *bodies);
int eoc_seeded_encrypt_bits_keyed(const eoc_secret_key *sk, const uint8_t enc_key[32], const uint8_t mask_seed[32],
                                  uint64_t first_idx, const uint8_t *bits, size_t count, int32_t *bodies);
int eoc_seeded_encrypt_ints_keyed(const eoc_secret_key *sk, const uint8_t enc_key[32], const uint8_t mask_seed[32],
                                  uint64_t first_idx, int p, const uint8_t *values, size_t count, int32_t *bodies);
int eoc_tgsw_seeded_encrypt_bits(const eoc_secret_key *sk, const uint8_t *bits, size_t count, uint8_t seed_out[32],
                                 int32_t *bodies);
int eoc_tgsw_seeded_encrypt_bits_keyed(const eoc_secret_key *sk, const uint8_t enc_key[32], const uint8_t mask_seed[32],
                                       uint64_t first_idx, const uint8_t *bits, size_t count, int32_t *bodies);
size_t eoc_seeded_cloud_key_blob_bytes(const eoc_params *p);
int eoc_seeded_cloud_key_export(const eoc_secret_key *sk, void *buf, size_t cap);   /* EOC_ERR_ARG when cap is too small */
int eoc_seeded_cloud_key_blob_params(const void *buf, size_t len, eoc_params *p);   /* a whole EOCCKS1 blob, else EOC_ERR_ARG */
int eoc_seeded_expand_host(const eoc_params *p, const uint8_t seed[32], uint64_t first_idx, const int32_t *bodies, size_t count,
                           int32_t *out);
int eoc_tgsw_seeded_expand_host(const eoc_params *p, const uint8_t seed[32], uint64_t first_idx, const int32_t *bodies,
                                size_t count, int32_t *out);
int eoc_seeded_cloud_key_expand(const void *blob, size_t len, int32_t *bk, int32_t *ksk);
int eoc_seeded_expand_device(eoc_engine *e, const uint8_t seed[32], uint64_t first_idx, const int32_t *d_bodies, size_t count,
                             int32_t *d_out, void *hip_stream);
int eoc_tgsw_seeded_to_fft_device(eoc_engine *e, const uint8_t seed[32], uint64_t first_idx, const int32_t *d_bodies,
                                  size_t count, void *d_fft, void *hip_stream);
int eoc_engine_load_seeded_cloud_key(eoc_engine *e, const void *blob, size_t len);
int eoc_engine_create_from_seeded_cloud_key_blob(int device, const void *blob, size_t len, eoc_engine **out);
uint64_t eoc_engine_seed_launches(eoc_engine *e);
int eoc_dbg_chacha20_blocks_device(eoc_engine *e, const uint8_t key[32], uint64_t counter, uint64_t nonce, size_t n_blocks,
                                   uint32_t *d_out, void *hip_stream);
int eoc_seeded_expand(const uint8_t seed[32], uint64_t first_idx, const int32_t *bodies, size_t count, int32_t *out);
int eoc_global_import_seeded_cloud_key_blob(const void *buf, size_t len);

/* ---- inner products with public integer weights on compact lists --------------------------------------------
 * A weighted sum of many encrypted values with PUBLIC weights, ready for one bootstrap: a dense layer of a discretised
 * network, a linear classifier, a score.  With the inputs packed in lists, an output costs one spectral multiply-add per
 * list, one inverse transform per 8 lists and ONE key switch -- not one key switch per input.
 *   weights     w[rows][cols] int8, every value in [-127, 127] (-128: EOC_ERR_ARG); weights past `cols` are zero.
 *               bias[rows] Torus32, optional.  rows, cols in [1, 2^20].
 *   inputs      `batch` vectors of L = ceil(cols / N) lists each, [batch][L][2][N] int32, c0 first: input k of a vector in slot
 *               k mod N of its list k / N (eoc_pk_encrypt_*, eoc_pack_device).
 *   output      for every (vector b, row r) one LWE sample of dimension N under s', [N+1] -- what eoc_blind_rotate_device
 *               emits and eoc_keyswitch_device takes -- of phase bias[r] + sum_k w[r][k] phase(slot k of vector b).
 *   rule        wrapping 32-bit arithmetic.  Weight polynomial V of (r, l): V[0] = w[r][lN], V[N - k] = -w[r][lN + k];
 *               coefficient 0 of V C is sum_k w_k C[k].  Body b' = bias[r] + sum_k w[r][k] c1_b[k], an exact integer sum.
 *               Mask: P0 = sum_l V_{r,l} c0_{b,l}, a'_0 = P0[0], a'_i = -P0[N - i].  The products are negacyclic products in
 *               the canonical transform: weight spectrum = the unscaled forward transform of V, list spectrum = the forward
 *               transform at scale 2^-9 (eoc_tgsw_to_fft_device's image), accumulated list by list (ascending) in the chains'
 *               nesting, the weight spectrum in the digit's place.  8 consecutive lists are a CHUNK: one inverse transform and
 *               conversion per chunk (8 * 1024 * 127 * 2^31 < 2^51: the conversion's contract holds for every input); chunks
 *               combine by integer addition.  The chunk is part of the format: eoc_dot_device equals the CPU reference
 *               tests/c/dot_ref.c byte for byte, and the exact product up to the conversion's few units per chunk.
 *   image       eoc_weights_to_device builds the model's device image once: the weight spectra [rows][L][512] complex f64
 *               (sigma order, as every image), then the weights [rows][L N] int8, zero-padded; eoc_weights_image_bytes(rows,
 *               cols) = rows L (8192 + 1024) bytes (0 for a shape that is refused).  A model load: checked on the host, no key,
 *               allocates a staging buffer and drains `hip_stream` (EOC_ERR_STATE under capture).
 *   noise       noise.linear_var = |w|^2 x the per-slot variance (the mean over rows of independent weights; one fixed row under
 *               one key: noise.linear_var_row, exact); for fresh lists the fixed offset noise.linear_offset.
 *   security    nothing new: the weights are public, the inputs are the lists of DESIGN.md 11 and every step is a public
 *               linear map of them.
 *   engine      eoc_dot_device needs NO key and writes d_u DEVICE [batch][rows][N+1]; eoc_linear_device is the same operation
 *               followed by the key switch (EOC_ERR_NO_KEY without a cloud key), d_out DEVICE [batch][rows][n+1]: its mask
 *               kernel writes the key switch's operand rows directly.  batch x rows = 0 is a no-op; EOC_ERR_ARG when the
 *               output overlaps the lists, the image or the bias.  Workspace: the list spectra of a slice of whole vectors
 *               (16 KiB per list; budget EOC_TFHE_DOT_WS_BYTES, default 256 MiB; slices of at most 2^20 samples), grown as
 *               every workspace: EOC_ERR_STATE if it would grow under capture (run one call of the shape first;
 *               eoc_engine_reserve(batch x rows, 0, 0) for eoc_linear_device).  Arguments travel as kernel arguments: no
 *               descriptor ring slot.  eoc_engine_dot_launches counts one per slice; the key switches are counted in the
 *               stats; eoc_engine_kernel_times books the new kernels under the key switch.
 *   host        eoc_linear: host buffers on the global context (a cloud key alone suffices: key mode 2), synchronous; WHOLE
 *               input vectors are cut into eoc_shard_range blocks, one per engine; every engine builds the image itself.
 *   messages    eoc_pk_encrypt_torus(_keyed): lists of ARBITRARY Torus32 messages (int32 per slot), e.g. x_k Delta; the same
 *               streams, u, e1 and e2 as eoc_pk_encrypt_bits -- the bits' lists are those of the messages +-2^29. */
size_t eoc_weights_image_bytes(size_t rows, size_t cols);
int eoc_weights_to_device(eoc_engine *e, const int8_t *h_w, size_t rows, size_t cols, void *d_image, void *hip_stream);
int eoc_dot_device(eoc_engine *e, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists, size_t batch,
                   const int32_t *d_bias /* may be NULL */, int32_t *d_u, void *hip_stream);
int eoc_linear_device(eoc_engine *e, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists, size_t batch,
                      const int32_t *d_bias /* may be NULL */, int32_t *d_out, void *hip_stream);
uint64_t eoc_engine_dot_launches(eoc_engine *e);
int eoc_linear(const int8_t *h_w, size_t rows, size_t cols, const int32_t *h_lists, size_t batch,
               const int32_t *h_bias /* may be NULL */, int32_t *h_out);
int eoc_pk_encrypt_torus(const void *pk, size_t pk_len, uint64_t enc_seed, uint64_t first_list, const int32_t *msgs,
                         size_t count, int32_t *lists);
int eoc_pk_encrypt_torus_keyed(const void *pk, size_t pk_len, const uint8_t enc_key[32], uint64_t first_list,
                               const int32_t *msgs, size_t count, int32_t *lists);

/* ---- convolutions with public int8 kernels on compact lists ---------------------------------------------------
 * The inner product above keeps ONE coefficient of the product of a list with the weight polynomial; all N coefficients are
 * the N shifts of a filter over the list.  These calls keep them: a convolution layer of a discretised network, a FIR filter,
 * a sliding-window score.  Weights, image (eoc_weights_to_device, unchanged), lists and format rule are the inner product's.
 *   layout      rows = output channels; list l of a vector = input channel l (L = ceil(cols / N) channels); w[r][lN + k] = tap k
 *               of filter (r, l).  An image is stored row-major in one list per channel (height x width <= N): tap (i, j) of a
 *               2-D filter is tap i width + j.
 *   output      for every (vector b, row r) the whole TLWE list [2][N] int32, c0 first:
 *                   out[b][r] = ( sum_l V_{r,l} c0_{b,l} ,  bias[r] + sum_l V_{r,l} c1_{b,l} )
 *               slot t has phase bias[r] + sum_l sum_k w[r][lN + k] x_l[t + k]: a cross-correlation (the "conv" of machine
 *               learning).  Terms with t + k >= N enter as -w x_l[t + k - N]: the negacyclic wrap is part of the rule; a caller
 *               that wants a linear convolution of `len` inputs with K taps reads slots t <= len - K only.
 *   rule        both polynomials through the inner product's chunks: 8 lists, l ascending, weight spectrum in the digit's place,
 *               list spectrum (scale 2^-9) in the key row's, one inverse transform and one conversion per chunk and polynomial
 *               (8 * 1024 * 127 * 2^31 < 2^51 for both), chunks combine by wrapping integer addition, the bias is added to every
 *               word of c1.  Word j of out[b][r].c0 is mask word (N - j) mod N of eoc_dot_device's sample (b, r), negated for
 *               j > 0, bit for bit.  eoc_conv_device equals the CPU reference tests/c/conv_ref.c byte for byte, and the exact
 *               product up to the conversion's few units per chunk.
 *   slots       a slot table names the samples a caller wants: entry s is slot slots[s] mod N of list slots[s] / N of a vector's
 *               `rows` output lists, any order, repeats allowed, n_slots in [1, 2^20].  The run calls take the table as a DEVICE
 *               pointer and do not read it on the host.  eoc_conv_slots_to_device loads it, as eoc_weights_to_device loads a
 *               model: every entry is checked on the host against lists_per_vec x N (EOC_ERR_ARG), the copy drains `hip_stream`,
 *               EOC_ERR_STATE under capture.  A table that did not come through it is not checked by the run calls; the kernel
 *               holds a list index past the vector to its last list, so no table makes it read outside the vector.
 *   noise       slot t is the inner product with the row noise.conv_row(w_row, t): noise.linear_var, linear_var_row and
 *               linear_offset price it, nothing fitted.
 *   engine      eoc_conv_device needs NO key and returns compact lists: 8 KiB per 1 024 results.  eoc_conv_linear_device is the
 *               same operation into a scratch buffer, then the table's samples extracted and key-switched: d_out DEVICE
 *               [batch][n_slots][n+1] (EOC_ERR_NO_KEY without a cloud key).  eoc_conv_extract_device is the extraction and the
 *               key switch alone, on `lists_per_vec` lists per vector the caller holds.  batch x rows = 0 (batch x n_slots = 0) is
 *               a no-op; EOC_ERR_ARG for a null pointer, a shape outside [1, 2^20], an output that overlaps an input.
 *               Workspace: the list spectra (16 KiB per list) and, for eoc_conv_linear_device, the output lists (8 KiB per row)
 *               of a slice of whole vectors, together inside EOC_TFHE_DOT_WS_BYTES (default 256 MiB; slices of at most 2^20
 *               samples and 65 535 vectors); grown as every workspace: EOC_ERR_STATE if one would grow under capture (run one
 *               call of the shape first).  Arguments travel as kernel arguments: no descriptor ring slot; every run call can be
 *               captured.  eoc_engine_conv_launches counts one per slice; the key switches are counted in the stats;
 *               eoc_engine_kernel_times books the new kernels under the key switch.
 *   host        eoc_conv_linear: host buffers (the slot table too) on the global context (a cloud key alone suffices),
 *               synchronous; WHOLE input vectors are cut into eoc_shard_range blocks, one per engine; every engine builds the
 *               image and loads the table itself. */
int eoc_conv_slots_to_device(eoc_engine *e, const uint32_t *h_slots, size_t n_slots, size_t lists_per_vec, uint32_t *d_slots,
                             void *hip_stream);
int eoc_conv_device(eoc_engine *e, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists, size_t batch,
                    const int32_t *d_bias /* may be NULL */, int32_t *d_out_lists /* [batch][rows][2][N] */, void *hip_stream);
int eoc_conv_linear_device(eoc_engine *e, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists, size_t batch,
                           const int32_t *d_bias /* may be NULL */, const uint32_t *d_slots, size_t n_slots,
                           int32_t *d_out /* [batch][n_slots][n+1] */, void *hip_stream);
int eoc_conv_extract_device(eoc_engine *e, const int32_t *d_lists, size_t lists_per_vec, size_t batch, const uint32_t *d_slots,
                            size_t n_slots, int32_t *d_out /* [batch][n_slots][n+1] */, void *hip_stream);
uint64_t eoc_engine_conv_launches(eoc_engine *e);
int eoc_conv_linear(const int8_t *h_w, size_t rows, size_t cols, const int32_t *h_lists, size_t batch,
                    const int32_t *h_bias /* may be NULL */, const uint32_t *h_slots, size_t n_slots, int32_t *h_out);

#ifdef __cplusplus
}
#endif
#endif /* EOC_TFHE_GPU_H */
