// cmaes.hip -- the (mu/mu_w, lambda)-CMA-ES of st_ito/cmaes.py with its state on the device: ask, tell and the eigendecomposition
// as float64 kernels, so that a whole run_es call is a stream of launches (stito_cmaes_*, ABI 10.6).
//
// The update rule is CMAEvolutionStrategy._ask / ._tell and _EsRun.tell, statement by statement; the two sides differ in the order of
// float64 sums only.  Everything but ask is ONE workgroup: N <= 128 and lambda <= 1024 fit one CU, and a single workgroup needs no
// atomics and no grid barrier.  ask is one workgroup per candidate (its rows are independent).
//
// The state is one allocation of 8-byte words laid out by cma_layout() -- the size query, the kernels, init, import and export all go
// through it.  A state that is `stopped` (early stop) or has logged max_iters iterations is FROZEN: ask, tell and the decomposition
// return without a store, so what a run computes does not depend on how many iterations the host enqueued past the freeze.
#include "common.h"

#include <atomic>
#include <cmath>
#include <vector>

namespace stito {

// ---- layout --------------------------------------------------------------------------------------------------------------------
enum { CI_DONE = 0, CI_STALE, CI_STOPPED, CI_COUNTEVAL, CI_COUNTITER, CI_EIGENEVAL, CI_BEST_EVALS, CI_N, CI_LAM, CI_MU, CI_MAX_ITERS,
       CI_EARLY_STOP, CI_SEED, CI_TOLD, CI_NEED_EIG, CI_SWEEPS, CI_ASKED, CI_COUNT };
enum { CR_SIGMA = 0, CR_BEST_F, CR_CC, CR_CS, CR_C1, CR_CMU, CR_DAMPS, CR_MUEFF, CR_CHIN, CR_LB, CR_UB, CR_AL, CR_AU, CR_WSUM, CR_HSIG,
       CR_SIGMA0, CR_COUNT };
constexpr int CMA_DISP = 8;   // words per row of the per-iteration log: countiter, counteval, f of the iteration's best, axis ratio,
                              // sigma, min std, max std, hsig
constexpr int CMA_FIELDS = 18;
constexpr int CMA_MAX_DEVICES = 64;

// offsets in 8-byte words; [0, persist) is what import / export move, the rest is scratch
struct CmaLayout {
    long long ints, reals, mean, pc, ps, D, best_x, weights, C, B, invC, geno, log_f, log_x, log_disp, persist, ys, tmp, total;
};

__host__ __device__ static inline CmaLayout cma_layout(long long N, long long lam, long long iters) {
    CmaLayout L;
    long long o = 0;
    auto add = [&o](long long n) { const long long at = o; o += n; return at; };
    L.ints = add(CI_COUNT);
    L.reals = add(CR_COUNT);
    L.mean = add(N); L.pc = add(N); L.ps = add(N); L.D = add(N); L.best_x = add(N);
    L.weights = add(lam);
    L.C = add(N * N); L.B = add(N * N); L.invC = add(N * N);
    L.geno = add(lam * N);
    L.log_f = add(iters); L.log_x = add(iters * N); L.log_disp = add(iters * CMA_DISP);
    L.persist = o;
    L.ys = add(lam * N);     // the sorted steps Y of a tell
    L.tmp = add(N * N);      // second buffer of the Jacobi rounds when two do not fit the LDS
    L.total = o;
    return L;
}

static int cma_check_dims(int N, int lam, long long iters) {
    STITO_REQUIRE(N >= 2 && N <= 128, STITO_E_UNSUPPORTED, "device CMA-ES: N = %d is outside the supported 2 .. 128", N);
    STITO_REQUIRE(lam >= 2 && lam <= 1024, STITO_E_UNSUPPORTED, "device CMA-ES: popsize %d is outside the supported 2 .. 1024", lam);
    STITO_REQUIRE(iters >= 1 && iters <= (1 << 20), STITO_E_INVALID, "device CMA-ES: max_iters %lld is outside 1 .. 2^20", iters);
    return STITO_OK;
}

// ---- the generator: splitmix64 read at random access ---------------------------------------------------------------------------
// bits(seed, iteration, e) = output e of the splitmix64 stream whose state starts at mix(mix(seed) ^ iteration): a pure function of
// its three arguments.  The deviate is Box-Muller's cosine branch on the two 32-bit halves, one 64-bit word per deviate.
__host__ __device__ static inline unsigned long long cma_mix(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ static inline unsigned long long cma_bits(unsigned long long seed, unsigned long long iteration, unsigned long long e) {
    const unsigned long long key = cma_mix(cma_mix(seed) ^ iteration);
    return cma_mix(key + e * 0x9E3779B97F4A7C15ull);
}
__device__ static inline double cma_normal(unsigned long long bits) {
    const double u1 = ((double)(bits >> 32) + 0.5) * (1.0 / 4294967296.0);
    const double u2 = ((double)(bits & 0xFFFFFFFFull) + 0.5) * (1.0 / 4294967296.0);
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// BoundTransform.__call__ for one value
__device__ static inline double cma_bound(double y, double lb, double ub, double al, double au) {
    const double lo = lb - al, hi = ub + au;
    if (y < lo || y > hi) {
        const double period = 2.0 * (hi - lo);
        double r = fmod(y - lo, period);   // np.mod: the remainder takes the divisor's sign
        if (r < 0.0) r += period;
        const double v = lo + r;
        y = v > hi ? 2.0 * hi - v : v;
    }
    if (y < lb + al) { const double d = y - (lb - al); return lb + d * d / (4.0 * al); }
    if (y > ub - au) { const double d = y - (ub + au); return ub - d * d / (4.0 * au); }
    return y;
}

__device__ static inline bool cma_frozen(const long long *ci) { return ci[CI_STOPPED] != 0 || ci[CI_DONE] >= ci[CI_MAX_ITERS]; }

__global__ __launch_bounds__(256) void k_cma_normals(unsigned long long seed, unsigned long long iteration, long long first, long long count,
                                                     double *z, unsigned long long *bits) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const unsigned long long b = cma_bits(seed, iteration, (unsigned long long)(first + i));
        if (bits != nullptr) bits[i] = b;
        if (z != nullptr) z[i] = cma_normal(b);
    }
}

// ---- ask: one workgroup per candidate ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_cma_ask(double *S, int N, int lam, long long iters, const double *z, double *W) {
    const CmaLayout L = cma_layout(N, lam, iters);
    const long long *ci = (const long long *)(S + L.ints);
    if (cma_frozen(ci)) return;
    const double *cr = S + L.reals;
    __shared__ double zd[128];
    const int k = blockIdx.x, j = threadIdx.x;
    if (k == 0 && j == 0) ((long long *)(S + L.ints))[CI_ASKED] = 1;   // (no workgroup of this launch reads it)
    if (j < N) {
        const long long e = (long long)k * N + j;
        const double zz = z != nullptr ? z[e] : cma_normal(cma_bits((unsigned long long)ci[CI_SEED], (unsigned long long)ci[CI_COUNTITER],
                                                                    (unsigned long long)e));
        zd[j] = zz * S[L.D + j];
    }
    __syncthreads();
    if (j < N) {
        const double *Bj = S + L.B + (long long)j * N;
        double y = 0.0;
        for (int i = 0; i < N; ++i) y += zd[i] * Bj[i];
        const double g = S[L.mean + j] + cr[CR_SIGMA] * y;
        S[L.geno + (long long)k * N + j] = g;
        W[(long long)k * N + j] = cma_bound(g, cr[CR_LB], cr[CR_UB], cr[CR_AL], cr[CR_AU]);
    }
}

// ---- tell: one workgroup -------------------------------------------------------------------------------------------------------
constexpr int TELL_THREADS = 1024;

__global__ __launch_bounds__(TELL_THREADS) void k_cma_tell(double *S, int N, int lam, long long iters, const float *fit) {
    const CmaLayout L = cma_layout(N, lam, iters);
    long long *ci = (long long *)(S + L.ints);
    // no ask pending: the genotype words are spent (they hold the last tell's squared components), nothing to learn from them
    if (cma_frozen(ci) || ci[CI_ASKED] == 0) return;
    double *cr = S + L.reals;
    __shared__ double f[1024], wo[1024];
    __shared__ int order[1024];
    __shared__ double ym[128], oldm[128], red[128], sc[2];
    const int t = threadIdx.x;
    const int mu = (int)ci[CI_MU];
    const long long it = ci[CI_DONE], counteval0 = ci[CI_COUNTEVAL], countiter = ci[CI_COUNTITER] + 1;
    const double sigma = cr[CR_SIGMA], best_before = cr[CR_BEST_F];
    const double cc = cr[CR_CC], cs = cr[CR_CS], c1 = cr[CR_C1], cmu = cr[CR_CMU], mueff = cr[CR_MUEFF], chiN = cr[CR_CHIN];
    if (t < lam) f[t] = (double)fit[t];
    __syncthreads();
    // rank of candidate t under np.argsort(kind="stable"): ascending, NaN last, ties in index order
    if (t < lam) {
        const double fk = f[t];
        const bool nank = fk != fk;
        int r = 0;
        for (int j = 0; j < lam; ++j) {
            const double fj = f[j];
            const bool nanj = fj != fj;
            r += nank ? (!nanj || j < t) : (!nanj && (fj < fk || (fj == fk && j < t)));
        }
        order[r] = t;
    }
    __syncthreads();
    const int k0 = order[0];
    const double f0 = f[k0];
    // the log holds the best BEFORE this tell (_EsRun.tell), then the best-so-far moves
    if (t < N) {
        S[L.log_x + it * N + t] = S[L.best_x + t];
        if (f0 < best_before) S[L.best_x + t] = cma_bound(S[L.geno + (long long)k0 * N + t], cr[CR_LB], cr[CR_UB], cr[CR_AL], cr[CR_AU]);
    }
    // weighted recombination
    if (t < N) {
        const double old = S[L.mean + t];
        double m = 0.0;
        for (int i = 0; i < mu; ++i) m += S[L.weights + i] * S[L.geno + (long long)order[i] * N + t];
        S[L.mean + t] = m;
        oldm[t] = old;
        ym[t] = (m - old) / sigma;
    }
    __syncthreads();
    if (t < N) {
        const double *row = S + L.invC + (long long)t * N;
        double v = 0.0;
        for (int i = 0; i < N; ++i) v += row[i] * ym[i];
        const double p = (1.0 - cs) * S[L.ps + t] + sqrt(cs * (2.0 - cs) * mueff) * v;
        S[L.ps + t] = p;
        red[t] = p * p;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += red[i];
        const double psn = sqrt(s);
        sc[0] = psn;
        sc[1] = (psn / sqrt(1.0 - pow(1.0 - cs, (double)(2 * countiter))) / chiN) < (1.4 + 2.0 / (N + 1)) ? 1.0 : 0.0;
    }
    __syncthreads();
    const double psn = sc[0];
    const bool hsig = sc[1] != 0.0;
    if (t < N) S[L.pc + t] = (1.0 - cc) * S[L.pc + t] + (hsig ? sqrt(cc * (2.0 - cc) * mueff) * ym[t] : 0.0);
    // the steps in rank order
    for (int e = t; e < lam * N; e += TELL_THREADS) {
        const int i = e / N, j = e - i * N;
        S[L.ys + e] = (S[L.geno + (long long)order[i] * N + j] - oldm[j]) / sigma;
    }
    __syncthreads();
    // Tutorial eq. (46): squared Mahalanobis norms of the steps with a negative weight; the genotypes are spent, their words hold
    // the squared components until the next ask
    for (int e = t; e < lam * N; e += TELL_THREADS) {
        const int i = e / N, j = e - i * N;
        if (S[L.weights + i] < 0.0) {
            const double *yi = S + L.ys + (long long)i * N, *row = S + L.invC + (long long)j * N;
            double v = 0.0;
            for (int k = 0; k < N; ++k) v += yi[k] * row[k];
            S[L.geno + e] = v * v;
        }
    }
    __syncthreads();
    if (t < lam) {
        double w = S[L.weights + t];
        if (w < 0.0) {
            double m = 0.0;
            for (int j = 0; j < N; ++j) m += S[L.geno + (long long)t * N + j];
            w = w * N / fmax(m, 1e-300);
        }
        wo[t] = w;
    }
    __syncthreads();
    const double dh = (hsig ? 0.0 : 1.0) * cc * (2.0 - cc);
    const double keep = 1.0 + c1 * dh - c1 - cmu * cr[CR_WSUM];
    for (int e = t; e < N * N; e += TELL_THREADS) {
        const int a = e / N, b = e - a * N;
        double s = 0.0;
        for (int i = 0; i < lam; ++i) s += (S[L.ys + (long long)i * N + a] * wo[i]) * S[L.ys + (long long)i * N + b];
        S[L.C + e] = keep * S[L.C + e] + c1 * (S[L.pc + a] * S[L.pc + b]) + cmu * s;
    }
    if (t == 0) {
        const double sigma_new = sigma * exp(fmin(1.0, (cs / cr[CR_DAMPS]) * (psn / chiN - 1.0)));
        const long long counteval = counteval0 + lam;
        S[L.log_f + it] = best_before;
        if (f0 < best_before) { cr[CR_BEST_F] = f0; ci[CI_BEST_EVALS] = counteval0 + k0 + 1; }
        cr[CR_SIGMA] = sigma_new;
        cr[CR_HSIG] = hsig ? 1.0 : 0.0;
        ci[CI_COUNTEVAL] = counteval;
        ci[CI_COUNTITER] = countiter;
        if ((double)(counteval - ci[CI_EIGENEVAL]) > (double)lam / (c1 + cmu) / N / 10.0) { ci[CI_EIGENEVAL] = counteval; ci[CI_NEED_EIG] = 1; }
        // _EsRun.tell: stale when the iteration's best did not beat the best on record by more than 0.01; never in iteration 0
        const bool stale = it > 0 && (f0 - best_before > -0.01);
        const long long n_stale = stale ? ci[CI_STALE] + 1 : 0;
        ci[CI_STALE] = n_stale;
        ci[CI_DONE] = it + 1;
        if (ci[CI_EARLY_STOP] != 0 && n_stale > 10) ci[CI_STOPPED] = 1;
        ci[CI_ASKED] = 0;
        ci[CI_TOLD] = 1;   // the decomposition launch that follows finishes this iteration's log row, frozen or not
        double *row = S + L.log_disp + it * CMA_DISP;
        row[0] = (double)countiter; row[1] = (double)counteval; row[2] = f0; row[4] = sigma_new; row[7] = hsig ? 1.0 : 0.0;
    }
}

// ---- eigendecomposition: cyclic Jacobi, round-robin pairs, one workgroup -------------------------------------------------------
// A = B^T C B (nearly diagonal from one iteration to the next) is rotated to diagonal form while the same rotations go into B.  A round
// of the round-robin schedule holds ceil(N / 2) disjoint pairs; a fixed group of threads owns a pair for the round, computes its
// rotation once, applies it to the pair's two ROWS from buffer A into buffer A2 (barrier), then to the two COLUMNS from A2 back into A
// and to the columns of B (barrier): two barriers per round, and no element is read and written in the same phase.  A stays in LDS;
// the rotated copy V of B is in LDS too up to N = 81 and A2 up to N = 96 (3 * 81^2 * 8 B = 154 KiB, 2 * 96^2 * 8 B = 144 KiB of the
// CU's 160); above that they are the state's B and its scratch words.  With V in global memory every round waits for a round trip to
// L2 at its barrier: 0.53 ms for six sweeps at N = 36 against 0.43 with it in LDS, measured (profiles/device_es.txt).
constexpr int EIG_THREADS = 256;
constexpr int EIG_MAX_SWEEPS = 30;

__device__ static inline double eig_reduce(double v, double *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = EIG_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// (the placement is a template parameter so that every access has its address space at compile time: through a pointer chosen at
// run time they are flat loads, which cost the LDS-resident case an eighth of its time: 0.43 -> 0.38 ms)
template <bool a2_in_lds, bool v_in_lds>
__global__ __launch_bounds__(EIG_THREADS) void k_cma_eigen(double *S, int N, int lam, long long iters, int force) {
    extern __shared__ double lds[];
    const CmaLayout L = cma_layout(N, lam, iters);
    long long *ci = (long long *)(S + L.ints);
    const bool told = ci[CI_TOLD] != 0;
    const bool forced = force && !cma_frozen(ci);   // a frozen state is left as it is; the tell that froze it still gets its log row
    if (!told && !forced) return;
    const bool decompose = forced || ci[CI_NEED_EIG] != 0;
    const int t = threadIdx.x;
    const int NN = N * N;
    double *C = S + L.C, *B = S + L.B, *D = S + L.D;
    if (decompose) {
        double *red = lds, *A = lds + EIG_THREADS, *A2 = a2_in_lds ? A + NN : S + L.tmp, *V = v_in_lds ? A + 2 * NN : B;
        // the host's np.triu(C) + np.triu(C, 1).T: the upper triangle is the matrix
        for (int e = t; e < NN; e += EIG_THREADS) {
            const int i = e / N, j = e - i * N;
            if (i > j) C[e] = C[j * N + i];
            if (v_in_lds) V[e] = B[e];
        }
        __syncthreads();
        for (int e = t; e < NN; e += EIG_THREADS) {   // A2 = C B
            const int i = e / N, j = e - i * N;
            double s = 0.0;
            for (int k = 0; k < N; ++k) s += C[i * N + k] * B[k * N + j];
            A2[e] = s;
        }
        __syncthreads();
        double fro = 0.0;
        for (int e = t; e < NN; e += EIG_THREADS) {   // A = B^T A2, computed for i <= j and mirrored
            const int i = e / N, j = e - i * N;
            if (i <= j) {
                double s = 0.0;
                for (int k = 0; k < N; ++k) s += B[k * N + i] * A2[k * N + j];
                A[i * N + j] = s;
                A[j * N + i] = s;
                fro += (i == j ? 1.0 : 2.0) * s * s;
            }
        }
        __syncthreads();
        const double fro2 = eig_reduce(fro, red);
        const int n2 = (N + 1) & ~1, npairs = n2 / 2, tpp = EIG_THREADS / npairs;   // tpp >= 4
        const int k = t / tpp, sub = t - k * tpp;
        const bool active = k < npairs;
        int sweeps = 0;
        for (; sweeps < EIG_MAX_SWEEPS; ++sweeps) {
            double off = 0.0;
            for (int e = t; e < NN; e += EIG_THREADS) {
                const int i = e / N, j = e - i * N;
                if (i != j) off += A[e] * A[e];
            }
            if (eig_reduce(off, red) <= 1e-30 * fro2) break;
            for (int r = 0; r < n2 - 1; ++r) {
                int p = 0, q = -1;
                double c = 1.0, s = 0.0, npp = 0.0, nqq = 0.0;
                if (active) {
                    int a = r + k, b = r - k;   // players (r + k) and (r - k) mod n2 - 1; player n2 - 1 stays and meets r
                    if (a >= n2 - 1) a -= n2 - 1;
                    if (b < 0) b += n2 - 1;
                    if (k == 0) { a = n2 - 1; b = r; }
                    p = a < b ? a : b;
                    q = a < b ? b : a;
                    if (q >= N) q = -1;   // odd N: the pair with the dummy player is a bye
                    npp = A[p * N + p];
                    if (q >= 0) {
                        const double apq = A[p * N + q], aqq = A[q * N + q];
                        nqq = aqq;
                        if (apq != 0.0) {
                            const double theta = (aqq - npp) / (2.0 * apq);
                            const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                            c = 1.0 / sqrt(tt * tt + 1.0);
                            s = tt * c;
                            npp -= tt * apq;
                            nqq += tt * apq;
                        }
                    }
                }
                if (active) {   // rows: reads A, writes A2
                    for (int j = sub; j < N; j += tpp) {
                        const double x = A[p * N + j];
                        if (q >= 0) {
                            const double y = A[q * N + j];
                            A2[p * N + j] = c * x - s * y;
                            A2[q * N + j] = s * x + c * y;
                        } else {
                            A2[p * N + j] = x;
                        }
                    }
                }
                __syncthreads();
                if (active) {   // columns: reads A2, writes A and B
                    for (int i = sub; i < N; i += tpp) {
                        const double x = A2[i * N + p];
                        if (q >= 0) {
                            const double y = A2[i * N + q];
                            // the rotated pair's own 2 x 2 block is known exactly: the off-diagonal element is zero
                            A[i * N + p] = i == p ? npp : (i == q ? 0.0 : c * x - s * y);
                            A[i * N + q] = i == q ? nqq : (i == p ? 0.0 : s * x + c * y);
                            const double u = V[i * N + p], v = V[i * N + q];
                            V[i * N + p] = c * u - s * v;
                            V[i * N + q] = s * u + c * v;
                        } else {
                            A[i * N + p] = x;
                        }
                    }
                }
                __syncthreads();   // the next round reads A
            }
        }
        if (t < N) D[t] = sqrt(fmax(A[t * N + t], 1e-30));
        __syncthreads();
        for (int e = t; e < NN; e += EIG_THREADS) {   // invsqrtC = (B / D) B^T
            const int i = e / N, j = e - i * N;
            double s = 0.0;
            for (int k2 = 0; k2 < N; ++k2) s += (V[i * N + k2] / D[k2]) * V[j * N + k2];
            S[L.invC + e] = s;
            if (v_in_lds) B[e] = V[e];
        }
        if (t == 0) ci[CI_SWEEPS] = sweeps;
        __syncthreads();
    }
    if (t == 0) {
        if (told) {   // the rest of the iteration's log row: what disp() prints after the decomposition
            double dmin = D[0], dmax = D[0], smin = C[0], smax = C[0];
            for (int i = 1; i < N; ++i) {
                dmin = fmin(dmin, D[i]); dmax = fmax(dmax, D[i]);
                smin = fmin(smin, C[i * N + i]); smax = fmax(smax, C[i * N + i]);
            }
            const double sigma = S[L.reals + CR_SIGMA];
            double *row = S + L.log_disp + (ci[CI_DONE] - 1) * CMA_DISP;
            row[3] = dmax / dmin; row[5] = sigma * sqrt(smin); row[6] = sigma * sqrt(smax);
        }
        ci[CI_TOLD] = 0;
        ci[CI_NEED_EIG] = 0;
    }
}

static int cma_launch_eigen(double *S, int N, int lam, long long iters, int force, hipStream_t st) {
    const int a2_in_lds = N <= 96, v_in_lds = N <= 81, which = v_in_lds ? 0 : a2_in_lds ? 1 : 2;
    const size_t lds = sizeof(double) * (EIG_THREADS + (size_t)N * N * (v_in_lds ? 3 : a2_in_lds ? 2 : 1));
    auto kern = v_in_lds ? k_cma_eigen<true, true> : a2_in_lds ? k_cma_eigen<true, false> : k_cma_eigen<false, false>;
    // the LDS attribute once per instantiation and device, at the most that instantiation can ask for (N = 81, 96, 128): no
    // attribute call on the launch path after the first, none inside a capture that an eager launch has preceded
    static std::atomic<bool> have[3][CMA_MAX_DEVICES];
    int dev = 0;
    STITO_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= CMA_MAX_DEVICES || !have[which][dev].load(std::memory_order_acquire)) {
        const int n_max = which == 0 ? 81 : which == 1 ? 96 : 128;
        const size_t lds_max = sizeof(double) * (EIG_THREADS + (size_t)n_max * n_max * (3 - which));
        STITO_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        if (dev >= 0 && dev < CMA_MAX_DEVICES) have[which][dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(kern, dim3(1), dim3(EIG_THREADS), lds, st, S, N, lam, iters, force);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

}  // namespace stito

using namespace stito;

extern "C" int64_t stito_cmaes_state_bytes(int N, int lam, int64_t max_iters) {
    STITO_TRY(cma_check_dims(N, lam, max_iters));
    return cma_layout(N, lam, max_iters).total * 8;
}

extern "C" int stito_cmaes_state_offsets(int N, int lam, int64_t max_iters, int64_t *offsets, int n_offsets) {
    STITO_TRY(cma_check_dims(N, lam, max_iters));
    STITO_REQUIRE(offsets != nullptr && n_offsets >= CMA_FIELDS, STITO_E_INVALID, "stito_cmaes_state_offsets: room for %d offsets needed", CMA_FIELDS);
    const CmaLayout L = cma_layout(N, lam, max_iters);
    const long long o[CMA_FIELDS] = {L.ints, L.reals, L.mean, L.pc, L.ps, L.D, L.best_x, L.weights, L.C, L.B, L.invC, L.geno, L.log_f, L.log_x,
                                     L.log_disp, L.persist, CI_COUNT, CMA_DISP};
    for (int i = 0; i < CMA_FIELDS; ++i) offsets[i] = o[i];
    return CMA_FIELDS;
}

extern "C" int stito_cmaes_import(void *state_dev, int N, int lam, int64_t max_iters, const int64_t *ints_host, const double *reals_host,
                                  void *stream) {
    STITO_TRY(cma_check_dims(N, lam, max_iters));
    STITO_REQUIRE(state_dev && ints_host && reals_host, STITO_E_INVALID, "stito_cmaes_import: NULL pointer");
    STITO_REQUIRE(ints_host[CI_N] == N && ints_host[CI_LAM] == lam && ints_host[CI_MAX_ITERS] == max_iters && ints_host[CI_MU] == lam / 2 &&
                      ints_host[CI_DONE] >= 0 && ints_host[CI_DONE] <= max_iters,
                  STITO_E_INVALID, "stito_cmaes_import: the state's header (N %lld, popsize %lld, max_iters %lld, done %lld) is not one of (%d, %d, %lld)",
                  (long long)ints_host[CI_N], (long long)ints_host[CI_LAM], (long long)ints_host[CI_MAX_ITERS], (long long)ints_host[CI_DONE], N,
                  lam, (long long)max_iters);
    const CmaLayout L = cma_layout(N, lam, max_iters);
    hipStream_t st = (hipStream_t)stream;
    double *S = (double *)state_dev;
    STITO_HIP_CHECK(hipMemcpyAsync(S + L.ints, ints_host, sizeof(int64_t) * CI_COUNT, hipMemcpyHostToDevice, st));
    STITO_HIP_CHECK(hipMemcpyAsync(S + L.reals, reals_host, sizeof(double) * (L.persist - CI_COUNT), hipMemcpyHostToDevice, st));
    STITO_HIP_CHECK(hipStreamSynchronize(st));
    return STITO_OK;
}

extern "C" int stito_cmaes_export(const void *state_dev, int N, int lam, int64_t max_iters, int64_t *ints_host, double *reals_host, void *stream) {
    STITO_TRY(cma_check_dims(N, lam, max_iters));
    STITO_REQUIRE(state_dev && ints_host && reals_host, STITO_E_INVALID, "stito_cmaes_export: NULL pointer");
    const CmaLayout L = cma_layout(N, lam, max_iters);
    hipStream_t st = (hipStream_t)stream;
    const double *S = (const double *)state_dev;
    STITO_HIP_CHECK(hipMemcpyAsync(ints_host, S + L.ints, sizeof(int64_t) * CI_COUNT, hipMemcpyDeviceToHost, st));
    STITO_HIP_CHECK(hipMemcpyAsync(reals_host, S + L.reals, sizeof(double) * (L.persist - CI_COUNT), hipMemcpyDeviceToHost, st));
    STITO_HIP_CHECK(hipStreamSynchronize(st));
    return STITO_OK;
}

extern "C" int stito_cmaes_status(const void *state_dev, int64_t *status_host, void *stream) {
    STITO_REQUIRE(state_dev && status_host, STITO_E_INVALID, "stito_cmaes_status: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    STITO_HIP_CHECK(hipMemcpyAsync(status_host, state_dev, sizeof(int64_t) * 4, hipMemcpyDeviceToHost, st));   // the header's first words
    STITO_HIP_CHECK(hipStreamSynchronize(st));
    return STITO_OK;
}

extern "C" int stito_cmaes_init(void *state_dev, int N, int lam, const double *x0_host, double sigma0, double lb, double ub, uint64_t seed,
                                int64_t max_iters, int early_stop, void *stream) {
    STITO_TRY(cma_check_dims(N, lam, max_iters));
    STITO_REQUIRE(state_dev && x0_host, STITO_E_INVALID, "stito_cmaes_init: NULL pointer");
    STITO_REQUIRE(ub > lb && sigma0 > 0.0, STITO_E_INVALID, "stito_cmaes_init: bounds [%g, %g] or sigma0 %g are not usable", lb, ub, sigma0);
    const CmaLayout L = cma_layout(N, lam, max_iters);
    std::vector<double> img((size_t)L.persist, 0.0);
    int64_t ci[CI_COUNT] = {0};
    double *cr = img.data() + L.reals;
    // CMAEvolutionStrategy.__init__, in its order
    const int mu = lam / 2;
    std::vector<double> wp(lam);
    for (int i = 0; i < lam; ++i) wp[i] = std::log((lam + 1) / 2.0) - std::log((double)(i + 1));
    double ps1 = 0.0, ps2 = 0.0, ns1 = 0.0, ns2 = 0.0;
    bool neg_any = false;
    for (int i = 0; i < mu; ++i) { ps1 += wp[i]; ps2 += wp[i] * wp[i]; }
    for (int i = mu; i < lam; ++i) { ns1 += wp[i]; ns2 += wp[i] * wp[i]; neg_any = neg_any || wp[i] != 0.0; }
    const double mueff = ps1 * ps1 / ps2;
    const double mueff_neg = neg_any ? ns1 * ns1 / ns2 : 0.0;
    const double cc = (4 + mueff / N) / (N + 4 + 2 * mueff / N);
    const double cs = (mueff + 2) / (N + mueff + 3);
    const double c1 = 2.0 / ((N + 1.3) * (N + 1.3) + mueff);
    const double cmu = std::min(1 - c1, 2.0 * (0.25 + mueff + 1 / mueff - 2) / ((N + 2.0) * (N + 2.0) + 2.0 * mueff / 2));
    const double damps = 1 + 2 * std::max(0.0, std::sqrt((mueff - 1) / (N + 1)) - 1) + cs;
    double *w = img.data() + L.weights, wsum = 0.0;
    for (int i = 0; i < mu; ++i) w[i] = wp[i] / ps1;
    if (ns1 != 0.0) {
        const double a_mu = 1 + c1 / cmu, a_mueff = 1 + 2 * mueff_neg / (mueff + 2), a_posdef = (1 - c1 - cmu) / (N * cmu);
        const double scale = std::min(a_mu, std::min(a_mueff, a_posdef));
        for (int i = mu; i < lam; ++i) w[i] = scale * wp[i] / (-ns1);
    }
    for (int i = 0; i < lam; ++i) wsum += w[i];
    const double al = std::min((ub - lb) / 2.0, (1.0 + std::fabs(lb)) / 20.0), au = std::min((ub - lb) / 2.0, (1.0 + std::fabs(ub)) / 20.0);
    for (int j = 0; j < N; ++j) {   // BoundTransform.inverse
        const double x = std::min(std::max(x0_host[j], lb), ub);
        double y = x;
        if (x < lb + al) y = (lb - al) + 2.0 * std::sqrt(al * (x - lb));
        if (x > ub - au) y = (ub + au) - 2.0 * std::sqrt(au * (ub - x));
        img[L.mean + j] = y;
        img[L.D + j] = 1.0;
        img[L.C + (size_t)j * N + j] = img[L.B + (size_t)j * N + j] = img[L.invC + (size_t)j * N + j] = 1.0;
    }
    ci[CI_N] = N; ci[CI_LAM] = lam; ci[CI_MU] = mu; ci[CI_MAX_ITERS] = max_iters; ci[CI_EARLY_STOP] = early_stop ? 1 : 0;
    ci[CI_SEED] = (int64_t)seed;
    cr[CR_SIGMA] = sigma0; cr[CR_SIGMA0] = sigma0; cr[CR_BEST_F] = INFINITY;
    cr[CR_CC] = cc; cr[CR_CS] = cs; cr[CR_C1] = c1; cr[CR_CMU] = cmu; cr[CR_DAMPS] = damps; cr[CR_MUEFF] = mueff;
    cr[CR_CHIN] = std::sqrt((double)N) * (1 - 1.0 / (4 * N) + 1.0 / (21.0 * N * N));
    cr[CR_LB] = lb; cr[CR_UB] = ub; cr[CR_AL] = al; cr[CR_AU] = au; cr[CR_WSUM] = wsum;
    return stito_cmaes_import(state_dev, N, lam, max_iters, ci, img.data() + L.reals, stream);
}

extern "C" int stito_cmaes_ask(void *state_dev, int N, int lam, int64_t max_iters, const double *z_dev, double *W_dev, void *stream) {
    STITO_TRY(cma_check_dims(N, lam, max_iters));
    STITO_REQUIRE(state_dev && W_dev, STITO_E_INVALID, "stito_cmaes_ask: NULL pointer");
    hipLaunchKernelGGL(k_cma_ask, dim3(lam), dim3(128), 0, (hipStream_t)stream, (double *)state_dev, N, lam, (long long)max_iters, z_dev, W_dev);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

extern "C" int stito_cmaes_tell(void *state_dev, int N, int lam, int64_t max_iters, const float *fitness_dev, void *stream) {
    STITO_TRY(cma_check_dims(N, lam, max_iters));
    STITO_REQUIRE(state_dev && fitness_dev, STITO_E_INVALID, "stito_cmaes_tell: NULL pointer");
    hipLaunchKernelGGL(k_cma_tell, dim3(1), dim3(TELL_THREADS), 0, (hipStream_t)stream, (double *)state_dev, N, lam, (long long)max_iters,
                       fitness_dev);
    STITO_LAUNCH_CHECK();
    return cma_launch_eigen((double *)state_dev, N, lam, max_iters, 0, (hipStream_t)stream);
}

extern "C" int stito_cmaes_eigen(void *state_dev, int N, int lam, int64_t max_iters, void *stream) {
    STITO_TRY(cma_check_dims(N, lam, max_iters));
    STITO_REQUIRE(state_dev, STITO_E_INVALID, "stito_cmaes_eigen: NULL pointer");
    return cma_launch_eigen((double *)state_dev, N, lam, max_iters, 1, (hipStream_t)stream);
}

extern "C" int stito_cmaes_normals(uint64_t seed, int64_t iteration, int64_t first, int64_t count, double *z_dev, uint64_t *bits_dev, void *stream) {
    STITO_REQUIRE(first >= 0 && count >= 0 && iteration >= 0, STITO_E_INVALID, "stito_cmaes_normals: negative iteration, first or count");
    if (count == 0) return STITO_OK;
    const long long blocks = std::min<long long>((count + 255) / 256, 4096);
    hipLaunchKernelGGL(k_cma_normals, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (unsigned long long)seed,
                       (unsigned long long)iteration, (long long)first, (long long)count, z_dev, (unsigned long long *)bits_dev);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}
