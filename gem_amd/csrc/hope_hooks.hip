// hope_hooks.hip -- what the library exports around the HOPE solvers for tests and tools: the host eigensolver's setters and wrappers, the three
// building-block entry points (gemhip_hope_spmm / _gram / _tsgemm) and the fourteen gemhip_test_hope_* hooks: ten on the launch functions, four on
// what the solvers and set-ups compose of them (apply_S / apply_ST, cheb_filter, orth / orth_scaled, the two spectrum estimates).  No kernel here:
// every hook calls the function of hope_ops.hpp that the solvers call, on a local Hope.  Touching a hook recompiles this unit alone.
#include "hope_ops.hpp"
#include "sym_eig.hpp"

using namespace gemhip;

// ------------------------------------------------------------------ the host eigensolver
extern "C" int gemhip_set_sym_eig_callback(int (*fn)(int32_t, double *, double *)) { set_sym_eig_callback(fn); return GEMHIP_OK; }

extern "C" int gemhip_set_host_threads(int32_t threads, int32_t *in_effect_out)
{
    GEMHIP_REQUIRE(threads <= 16, "set_host_threads: at most 16 threads (got %d)", threads);
    set_eig_threads(threads);                       // <= 0: back to the default
    const int t = eig_threads_in_effect();
    if (in_effect_out) *in_effect_out = t;
    return GEMHIP_OK;
}

static int sym_eig_full(const char *who, void (*solver)(int, std::vector<double> &, std::vector<double> &), int32_t n, double *A_inout, double *w_out)
{
    GEMHIP_REQUIRE(n >= 1 && A_inout && w_out, "%s: bad arguments", who);
    std::vector<double> V(A_inout, A_inout + (size_t)n * n), w;
    solver(n, V, w);
    std::copy(V.begin(), V.end(), A_inout);
    std::copy(w.begin(), w.end(), w_out);
    return GEMHIP_OK;
}
extern "C" int gemhip_sym_eig_builtin(int32_t n, double *A_inout, double *w_out) { return sym_eig_full("sym_eig_builtin", sym_eig_impl, n, A_inout, w_out); }
extern "C" int gemhip_sym_eig(int32_t n, double *A_inout, double *w_out) { return sym_eig_full("sym_eig", sym_eig, n, A_inout, w_out); }

extern "C" int gemhip_sym_eig_top(int32_t n, double *A_inout, int32_t m, double *w_out, double *Z_out)
{
    GEMHIP_REQUIRE(n >= 1 && m >= 1 && m <= n && A_inout && w_out && Z_out, "sym_eig_top: bad arguments");
    std::vector<double> V(A_inout, A_inout + (size_t)n * n), w, Z;
    sym_eig_top_impl(n, V, m, w, Z);
    std::copy(w.begin(), w.end(), w_out);
    std::copy(Z.begin(), Z.end(), Z_out);
    return GEMHIP_OK;
}

// ------------------------------------------------------------------ the launch functions under the solvers' calling conventions
// Each helper uploads host blocks (every one with its full leading dimension, padding included), calls the launch function the solvers call on a
// local Hope, and copies the output block back whole, so a caller that filled the padding with a sentinel sees any write outside the logical
// columns.  A building-block entry point is its own argument check and the same helper with ld = width and offsets 0.
namespace {

// The hooks' CSR check.  Not check_csr_arrays (hope_host.hpp), which the solvers' entry points use: that one refuses n = 1, which the hooks take,
// and does not look at row_ptr between its two ends, where this one refuses a decreasing entry (scripts/asan/hope_host_driver.cpp, self_csr, shows both).
bool hook_csr_ok(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col)
{
    if (n < 1 || nnz < 0 || !row_ptr || (nnz > 0 && !col) || row_ptr[0] != 0 || row_ptr[n] != nnz) return false;
    for (int64_t i = 0; i < n; ++i) if (row_ptr[i + 1] < row_ptr[i]) return false;
    for (int64_t e = 0; e < nnz; ++e) if (col[e] < 0 || col[e] >= n) return false;
    return true;
}

void hook_upload(Hope &H, DevBuf<float> &d, const float *host, int ld)     // the whole H.n x ld block; a NULL block stays empty (its pointer NULL)
{
    if (host) HOPE_TRY(H, d.upload(host, (size_t)H.n * ld));
}

int hook_download(Hope &H, void *host, const void *dev, size_t bytes)      // blocking: the null stream's work is done when it returns
{
    HOPE_TRY(H, hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return H.err;
}

int spmm_block(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t variant, float alpha, int32_t b,
               const float *X_host, int32_t ldx, float wa, const float *W_host, int32_t ldw, float wb, const float *W2_host, int32_t ldw2, int32_t w_is_x,
               int32_t w2_is_y, float *Y_inout, int32_t ldy, int32_t *launched_out)
{
    Hope H;
    upload_csr_w(H, n, nnz, row_ptr, col, w, false);
    if (variant == 1) H.knobs.spmm16 = 0;
    if (variant >= 2) { H.knobs.spmm16 = 1; H.knobs.spmm16_u = variant; }
    DevBuf<float> dX, dW, dW2, dY;
    hook_upload(H, dX, X_host, ldx); hook_upload(H, dW, W_host, ldw); hook_upload(H, dW2, W2_host, ldw2); hook_upload(H, dY, Y_inout, ldy);
    const float *pW = w_is_x ? dX.get() : dW.get(); const int lw = w_is_x ? ldx : ldw;
    const float *pW2 = w2_is_y ? dY.get() : dW2.get(); const int lw2 = w2_is_y ? ldy : ldw2;
    spmm(H, false, alpha, dX, ldx, pW, lw, dY, ldy, b, wa, pW2, lw2, wb);
    if (launched_out) { launched_out[0] = H.last_spmm_c; launched_out[1] = H.last_spmm_u; }
    return hook_download(H, Y_inout, dY, (size_t)n * ldy * sizeof(float));
}

int gram_block(int64_t n, const float *X_host, int32_t ldx, int32_t xoff, int32_t m1, const float *Y_host, int32_t ldy, int32_t yoff, int32_t m2,
               double *G_host, float *Gf_host)
{
    Hope H; H.n = n;
    DevBuf<float> dX, dY, dGf;
    hook_upload(H, dX, X_host, ldx); hook_upload(H, dY, Y_host, ldy);
    const float *pY = Y_host ? dY.get() : dX.get(); const int ly = Y_host ? ldy : ldx;
    if (!Gf_host) {
        std::vector<double> G;
        gram(H, dX + xoff, ldx, m1, pY + yoff, ly, m2, G);
        if (!H.err) std::copy(G.begin(), G.end(), G_host);
        return H.err;
    }
    HOPE_TRY(H, dGf.reserve((size_t)m1 * m2));
    gram_launch(H, dX + xoff, ldx, m1, pY + yoff, ly, m2, dGf);
    if (hook_download(H, G_host, H.G, (size_t)m1 * m2 * sizeof(double))) return H.err;
    return hook_download(H, Gf_host, dGf, (size_t)m1 * m2 * sizeof(float));
}

int tsgemm_block(int64_t n, const float *X_host, int32_t ldx, int32_t xoff, int32_t m, const double *C_host, int32_t b2, float alpha, const float *Src_host,
                 int32_t lds, int32_t in_place, float *Out_inout, int32_t ldo)
{
    Hope H; H.n = n;
    DevBuf<float> dX, dS, dO;
    hook_upload(H, dX, X_host, ldx); hook_upload(H, dS, Src_host, lds); hook_upload(H, dO, Out_inout, ldo);
    std::vector<double> C(C_host, C_host + (size_t)m * b2);
    tsgemm(H, dX + xoff, ldx, m, C, b2, alpha, in_place ? dO.get() : dS.get(), in_place ? ldo : lds, dO, ldo);
    return hook_download(H, Out_inout, dO, (size_t)n * ldo * sizeof(float));
}

}  // namespace

// ------------------------------------------------------------------ building blocks, exposed for kernel-level parity tests
extern "C" int gemhip_hope_spmm(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float alpha, int32_t b,
                                const float *X_host, const float *Wadd_host, float *Y_host)
{
    GEMHIP_REQUIRE(n >= 1 && row_ptr && X_host && Y_host && b >= 1 && b <= 512, "hope_spmm: bad arguments");
    return spmm_block(n, nnz, row_ptr, col, w, 0, alpha, b, X_host, b, 1.0f, Wadd_host, b, 0.f, nullptr, 0, 0, 0, Y_host, b, nullptr);
}

extern "C" int gemhip_hope_gram(int64_t n, int32_t m1, int32_t m2, const float *X_host, const float *Y_host, double *G_host)
{
    GEMHIP_REQUIRE(n >= 1 && m1 >= 1 && m2 >= 1 && X_host && Y_host && G_host, "hope_gram: bad arguments");
    return gram_block(n, X_host, m1, 0, m1, Y_host, m2, 0, m2, G_host, nullptr);
}

extern "C" int gemhip_hope_tsgemm(int64_t n, int32_t m, int32_t b2, const float *X_host, const double *C_host, float alpha, const float *Src_host,
                                  float *Out_host)
{
    GEMHIP_REQUIRE(n >= 1 && m >= 1 && b2 >= 1 && X_host && C_host && Out_host, "hope_tsgemm: bad arguments");
    return tsgemm_block(n, X_host, m, 0, m, C_host, b2, alpha, Src_host, b2, 0, Out_host, b2);
}

// ------------------------------------------------------------------ test hooks
// variant: 0 = the production dispatch, 1 = hope_spmm_kernel (one row per wavefront), 2 / 4 / 8 = hope_spmm16_kernel with that U.
// w_is_x: Wadd is the device block of X itself (ldw = ldx); w2_is_y: W2 is the device block of Y itself (Y_inout's contents, ldw2 = ldy).
// launched_out (may be NULL): the instantiation spmm() chose, {CPL16, U} or {CPL, 0}.
extern "C" int gemhip_test_hope_spmm(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t variant, float alpha,
                                     int32_t b, const float *X_host, int32_t ldx, float wa, const float *W_host, int32_t ldw, float wb,
                                     const float *W2_host, int32_t ldw2, int32_t w_is_x, int32_t w2_is_y, float *Y_inout, int32_t ldy,
                                     int32_t *launched_out)
{
    GEMHIP_REQUIRE(hook_csr_ok(n, nnz, row_ptr, col), "test_hope_spmm: bad CSR arguments");
    GEMHIP_REQUIRE(X_host && Y_inout && b >= 1 && b <= 512 && ldx >= b && ldy >= b, "test_hope_spmm: bad block arguments");
    GEMHIP_REQUIRE(variant == 0 || variant == 1 || ((variant == 2 || variant == 4 || variant == 8) && b <= 128), "test_hope_spmm: variant %d", variant);
    GEMHIP_REQUIRE(!(w_is_x && W_host) && !(w2_is_y && W2_host) && (!W_host || ldw >= b) && (!W2_host || ldw2 >= b), "test_hope_spmm: bad addend arguments");
    return spmm_block(n, nnz, row_ptr, col, w, variant, alpha, b, X_host, ldx, wa, W_host, ldw, wb, W2_host, ldw2, w_is_x, w2_is_y, Y_inout, ldy, launched_out);
}

// G[m1][m2] = X[:, xoff : xoff + m1]^T Y[:, yoff : yoff + m2]; Y_host NULL: Y is the device block of X (ldy = ldx).  Gf_host (may be NULL) receives
// the fp32 rounding hope_reduce2_kernel writes for project_out.
extern "C" int gemhip_test_hope_gram(int64_t n, const float *X_host, int32_t ldx, int32_t xoff, int32_t m1, const float *Y_host, int32_t ldy, int32_t yoff,
                                     int32_t m2, double *G_host, float *Gf_host)
{
    GEMHIP_REQUIRE(n >= 1 && X_host && G_host && m1 >= 1 && m2 >= 1 && xoff >= 0 && yoff >= 0 && xoff + m1 <= ldx && yoff + m2 <= (Y_host ? ldy : ldx),
                   "test_hope_gram: bad arguments");
    return gram_block(n, X_host, ldx, xoff, m1, Y_host, ldy, yoff, m2, G_host, Gf_host);
}

// gram2: Ga = Xa[:, xaoff : +ma1]^T Ya[:, yaoff : +ma2] and Gb likewise, in one call (shared scratch, one host round trip)
extern "C" int gemhip_test_hope_gram2(int64_t n, const float *Xa_host, int32_t ldxa, int32_t xaoff, int32_t ma1, const float *Ya_host, int32_t ldya,
                                      int32_t yaoff, int32_t ma2, double *Ga_host, const float *Xb_host, int32_t ldxb, int32_t xboff, int32_t mb1,
                                      const float *Yb_host, int32_t ldyb, int32_t yboff, int32_t mb2, double *Gb_host)
{
    GEMHIP_REQUIRE(n >= 1 && Xa_host && Ya_host && Xb_host && Yb_host && Ga_host && Gb_host, "test_hope_gram2: NULL argument");
    GEMHIP_REQUIRE(ma1 >= 1 && ma2 >= 1 && mb1 >= 1 && mb2 >= 1 && xaoff >= 0 && yaoff >= 0 && xboff >= 0 && yboff >= 0 && xaoff + ma1 <= ldxa &&
                   yaoff + ma2 <= ldya && xboff + mb1 <= ldxb && yboff + mb2 <= ldyb, "test_hope_gram2: bad shapes");
    Hope H; H.n = n;
    DevBuf<float> dXa, dYa, dXb, dYb;
    hook_upload(H, dXa, Xa_host, ldxa); hook_upload(H, dYa, Ya_host, ldya); hook_upload(H, dXb, Xb_host, ldxb); hook_upload(H, dYb, Yb_host, ldyb);
    std::vector<double> Ga, Gb;
    gram2(H, dXa + xaoff, ldxa, ma1, dYa + yaoff, ldya, ma2, Ga, dXb + xboff, ldxb, mb1, dYb + yboff, ldyb, mb2, Gb);
    if (!H.err) { std::copy(Ga.begin(), Ga.end(), Ga_host); std::copy(Gb.begin(), Gb.end(), Gb_host); }
    return H.err;
}

// Out[:, :b2] = (Src or 0) + alpha X[:, xoff : xoff + m] C.  in_place: Src is the device block of Out (Out_inout's contents, lds = ldo).
extern "C" int gemhip_test_hope_tsgemm(int64_t n, const float *X_host, int32_t ldx, int32_t xoff, int32_t m, const double *C_host, int32_t b2, float alpha,
                                       const float *Src_host, int32_t lds, int32_t in_place, float *Out_inout, int32_t ldo)
{
    GEMHIP_REQUIRE(n >= 1 && m >= 1 && b2 >= 1 && X_host && C_host && Out_inout && xoff >= 0 && xoff + m <= ldx && ldo >= b2, "test_hope_tsgemm: bad arguments");
    GEMHIP_REQUIRE(!(in_place && Src_host) && (!Src_host || lds >= b2), "test_hope_tsgemm: bad Src arguments");
    return tsgemm_block(n, X_host, ldx, xoff, m, C_host, b2, alpha, Src_host, lds, in_place, Out_inout, ldo);
}

// ritz_rotate: Out[:, :b2] = V[:, voff : +m] C, res2[j] = || B[:, boff : +m] C[:, j] - theta[j] Out[:, j] ||^2
extern "C" int gemhip_test_hope_ritz(int64_t n, const float *V_host, int32_t ldv, int32_t voff, const float *B_host, int32_t ldb, int32_t boff, int32_t m,
                                     const double *C_host, const double *theta_host, int32_t b2, float *Out_inout, int32_t ldo, double *res2_out)
{
    GEMHIP_REQUIRE(n >= 1 && m >= 1 && b2 >= 1 && V_host && B_host && C_host && theta_host && Out_inout && res2_out, "test_hope_ritz: bad arguments");
    GEMHIP_REQUIRE(voff >= 0 && boff >= 0 && voff + m <= ldv && boff + m <= ldb && ldo >= b2, "test_hope_ritz: bad shapes");
    Hope H; H.n = n;
    DevBuf<float> dV, dB, dO;
    hook_upload(H, dV, V_host, ldv); hook_upload(H, dB, B_host, ldb); hook_upload(H, dO, Out_inout, ldo);
    const std::vector<double> C(C_host, C_host + (size_t)m * b2), theta(theta_host, theta_host + b2);
    std::vector<double> res2;
    ritz_rotate(H, dV + voff, ldv, dB + boff, ldb, m, C, theta, b2, dO, ldo, res2);
    if (!H.err) std::copy(res2.begin(), res2.end(), res2_out);
    return hook_download(H, Out_inout, dO, (size_t)n * ldo * sizeof(float));
}

// colmax: val[j] = the entry of X[:, j] (j < mc) with the largest magnitude, first row on ties.  variant: 0 = production choice, 1 = one pass
// (hope_colmax_kernel), 2 = two passes (hope_colmax1/2_kernel).
extern "C" int gemhip_test_hope_colmax(int64_t n, const float *X_host, int32_t ld, int32_t mc, int32_t variant, float *val_out)
{
    GEMHIP_REQUIRE(n >= 1 && X_host && val_out && mc >= 1 && ld >= mc && variant >= 0 && variant <= 2, "test_hope_colmax: bad arguments");
    Hope H; H.n = n;
    if (variant) H.knobs.colmax2 = variant - 1;
    DevBuf<float> dX, dv;
    hook_upload(H, dX, X_host, ld);
    HOPE_TRY(H, dv.reserve(mc));
    colmax(H, dX, ld, mc, dv);
    return hook_download(H, val_out, dv, (size_t)mc * sizeof(float));
}

// project_out: W[:, :cols] -= V[:, :m] (V[:, :m]^T W[:, :cols]).  woff < 0: W_inout is its own n x ldw block.  woff >= 0: as in the solvers, W is the
// column block [woff, woff + cols) of V's own block (W = V + woff, ldw = ldv) and W_inout (n x ldv) receives that whole block back.
extern "C" int gemhip_test_hope_project_out(int64_t n, const float *V_host, int32_t ldv, int32_t m, float *W_inout, int32_t ldw, int32_t cols, int32_t woff)
{
    GEMHIP_REQUIRE(n >= 1 && V_host && W_inout && m >= 1 && cols >= 1 && m <= ldv && cols <= ldw, "test_hope_project_out: bad arguments");
    GEMHIP_REQUIRE(woff < 0 || (woff >= m && woff + cols <= ldv && ldw == ldv), "test_hope_project_out: bad shared block");
    Hope H; H.n = n;
    DevBuf<float> dV, dW;
    hook_upload(H, dV, V_host, ldv);
    if (woff < 0) hook_upload(H, dW, W_inout, ldw);
    project_out(H, dV, ldv, m, woff < 0 ? dW.get() : dV.get() + woff, ldw, cols);
    return hook_download(H, W_inout, woff < 0 ? dW.get() : dV.get(), (size_t)n * ldw * sizeof(float));
}

// apply_sym_op: Out[:, :cols] = alpha Op X + wa W + wb W2; kind 0: Op = the CSR matrix, kind 2: Op = (I - A)^T (I - A) (A as given: the caller
// normalises the rows).  The n x cols scratch of kind 2 is the hook's own.
extern "C" int gemhip_test_hope_sym_op(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t kind, float alpha,
                                       const float *X_host, int32_t ldx, int32_t cols, float wa, const float *W_host, int32_t ldw, float wb,
                                       const float *W2_host, int32_t ldw2, float *Out_inout, int32_t ldo)
{
    GEMHIP_REQUIRE(hook_csr_ok(n, nnz, row_ptr, col), "test_hope_sym_op: bad CSR arguments");
    GEMHIP_REQUIRE((kind == 0 || kind == 2) && X_host && Out_inout && cols >= 1 && cols <= 512 && ldx >= cols && ldo >= cols, "test_hope_sym_op: bad arguments");
    GEMHIP_REQUIRE((!W_host || ldw >= cols) && (!W2_host || ldw2 >= cols), "test_hope_sym_op: bad addend arguments");
    Hope H;
    upload_csr_w(H, n, nnz, row_ptr, col, w, true);
    H.mode = kind;
    DevBuf<float> dX, dW, dW2, dT, dO;
    hook_upload(H, dX, X_host, ldx); hook_upload(H, dW, W_host, ldw); hook_upload(H, dW2, W2_host, ldw2);
    HOPE_TRY(H, dT.reserve((size_t)n * cols));
    hook_upload(H, dO, Out_inout, ldo);
    apply_sym_op(H, kind, alpha, dX, ldx, cols, dT, cols, dO, ldo, wa, dW, ldw, wb, dW2, ldw2);
    return hook_download(H, Out_inout, dO, (size_t)n * ldo * sizeof(float));
}

// lincomb: Out[:, :b] = a X + b2 Y + c Z.  out_is_x: Out is the device block of X (Out_inout's contents are X, ldx = ldo; X_host NULL).
extern "C" int gemhip_test_hope_lincomb(int64_t n, int32_t b, float a, const float *X_host, int32_t ldx, float b2, const float *Y_host, int32_t ldy, float c,
                                        const float *Z_host, int32_t ldz, int32_t out_is_x, float *Out_inout, int32_t ldo)
{
    GEMHIP_REQUIRE(n >= 1 && b >= 1 && Y_host && Z_host && Out_inout && ldy >= b && ldz >= b && ldo >= b, "test_hope_lincomb: bad arguments");
    GEMHIP_REQUIRE(out_is_x ? X_host == nullptr : (X_host != nullptr && ldx >= b), "test_hope_lincomb: X_host and out_is_x exclude each other");
    Hope H; H.n = n;
    DevBuf<float> dX, dY, dZ, dO;
    hook_upload(H, dX, X_host, ldx); hook_upload(H, dY, Y_host, ldy); hook_upload(H, dZ, Z_host, ldz); hook_upload(H, dO, Out_inout, ldo);
    lincomb(H, b, a, out_is_x ? dO.get() : dX.get(), out_is_x ? ldo : ldx, b2, dY, ldy, c, dZ, ldz, dO, ldo);
    return hook_download(H, Out_inout, dO, (size_t)n * ldo * sizeof(float));
}

// randn: X[:, :b] = the solvers' starting block for `seed`
extern "C" int gemhip_test_hope_randn(int64_t n, int32_t b, int32_t ld, uint64_t seed, float *X_inout)
{
    GEMHIP_REQUIRE(n >= 1 && b >= 1 && ld >= b && X_inout, "test_hope_randn: bad arguments");
    Hope H; H.n = n;
    DevBuf<float> dX;
    hook_upload(H, dX, X_inout, ld);
    randn(H, dX, b, ld, seed);
    return hook_download(H, X_inout, dX, (size_t)n * ld * sizeof(float));
}

// ------------------------------------------------------------------ test hooks, one layer up: what the solvers compose of the launch functions
// apply_S (transpose = 0) / apply_ST (transpose = 1) of the operator `mode` (Hope::mode; `beta` is Hope::beta: the Katz factor, or c of mode 2) on the
// CSR matrix as given: Out[:, :b] = S X or S^T X.  T0, T1 and W0 (n x ldt each) are the hook's own.
extern "C" int gemhip_test_hope_apply_s(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t mode, float beta,
                                        int32_t transpose, int32_t terms, int32_t b, const float *X_host, int32_t ldx, int32_t ldt, float *Out_inout,
                                        int32_t ldo)
{
    GEMHIP_REQUIRE(hook_csr_ok(n, nnz, row_ptr, col), "test_hope_apply_s: bad CSR arguments");
    GEMHIP_REQUIRE(mode >= 0 && mode <= 2 && (transpose == 0 || transpose == 1) && terms >= 0 && terms <= 400, "test_hope_apply_s: bad operator arguments");
    GEMHIP_REQUIRE(X_host && Out_inout && b >= 1 && b <= 512 && ldx >= b && ldt >= b && ldo >= b, "test_hope_apply_s: bad block arguments");
    Hope H;
    upload_csr_w(H, n, nnz, row_ptr, col, w, true);
    H.mode = mode; H.beta = beta;
    DevBuf<float> dX, dO, dT[3];                                              // T0, T1, W0
    hook_upload(H, dX, X_host, ldx); hook_upload(H, dO, Out_inout, ldo);
    for (DevBuf<float> &t : dT) { HOPE_TRY(H, t.reserve((size_t)n * ldt)); HOPE_TRY(H, hipMemsetAsync(t, 0, (size_t)n * ldt * sizeof(float), H.s)); }
    if (transpose) apply_ST(H, dX, ldx, b, terms, dT[0], dT[1], ldt, dO, ldo);
    else apply_S(H, dX, ldx, b, terms, dT[0], dT[1], dT[2], ldt, dO, ldo);
    return hook_download(H, Out_inout, dO, (size_t)n * ldo * sizeof(float));
}

// cheb_filter: V[:, :cols] <- T_m((Op - c I) / e) V[:, :cols], Op of `kind` (0: the CSR matrix; 2: (I - A)^T (I - A)) as in gemhip_test_hope_sym_op, with
// Q[:, :nl] (NULL when nl = 0) projected out of the two live terms every q degrees.  The three recurrence blocks and the kind-2 scratch (n x ldf) are the hook's own.
extern "C" int gemhip_test_hope_cheb_filter(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t kind, int32_t m,
                                            double c, double e, float *V_inout, int32_t ldv, int32_t cols, int32_t ldf, const float *Q_host, int32_t ldq,
                                            int32_t nl, int32_t q)
{
    GEMHIP_REQUIRE(hook_csr_ok(n, nnz, row_ptr, col), "test_hope_cheb_filter: bad CSR arguments");
    GEMHIP_REQUIRE((kind == 0 || kind == 2) && m >= 1 && m <= 1024 && e > 0.0 && std::isfinite(c) && std::isfinite(e), "test_hope_cheb_filter: bad filter arguments");
    GEMHIP_REQUIRE(V_inout && cols >= 1 && cols <= 512 && ldv >= cols && ldf >= cols, "test_hope_cheb_filter: bad block arguments");
    GEMHIP_REQUIRE(nl >= 0 && q >= 0 && (nl == 0 || (Q_host && ldq >= nl)), "test_hope_cheb_filter: bad locked block");
    Hope H;
    upload_csr_w(H, n, nnz, row_ptr, col, w, true);
    H.mode = kind;
    DevBuf<float> dV, dQ, dF[4];                                              // F[0..2], Ts
    hook_upload(H, dV, V_inout, ldv);
    if (nl > 0) hook_upload(H, dQ, Q_host, ldq);
    for (DevBuf<float> &f : dF) { HOPE_TRY(H, f.reserve((size_t)n * ldf)); HOPE_TRY(H, hipMemsetAsync(f, 0, (size_t)n * ldf * sizeof(float), H.s)); }
    float *const F[3] = {dF[0].get(), dF[1].get(), dF[2].get()};
    cheb_filter(H, kind, dV, ldv, cols, m, c, e, F, ldf, dF[3], dQ, ldq, nl, q);
    return hook_download(H, V_inout, dV, (size_t)n * ldv * sizeof(float));
}

// orth (scaled = 0: tol, abs_floor, passes as the solvers pass them) or orth_scaled (scaled = 1: passes) on Y[:, :b] in place through an n x ldt scratch;
// keep_out receives the number of columns kept (columns [0, keep) of Y are the orthonormal block; the columns behind them keep what they held).
extern "C" int gemhip_test_hope_orth(int64_t n, float *Y_inout, int32_t ld, int32_t b, int32_t ldt, int32_t scaled, double tol, double abs_floor,
                                     int32_t passes, int32_t *keep_out)
{
    GEMHIP_REQUIRE(n >= 1 && Y_inout && keep_out && b >= 1 && b <= 512 && ld >= b && ldt >= b && passes >= 1 && passes <= 4 && (scaled == 0 || scaled == 1),
                   "test_hope_orth: bad arguments");
    Hope H; H.n = n;
    DevBuf<float> dY, dT;
    hook_upload(H, dY, Y_inout, ld);
    HOPE_TRY(H, dT.reserve((size_t)n * ldt));
    HOPE_TRY(H, hipMemsetAsync(dT, 0, (size_t)n * ldt * sizeof(float), H.s));
    const int keep = scaled ? orth_scaled(H, dY, ld, b, dT, ldt, passes) : orth(H, dY, ld, b, dT, ldt, tol, abs_floor, passes);
    *keep_out = H.err ? 0 : keep;
    return hook_download(H, Y_inout, dY, (size_t)n * ld * sizeof(float));
}

// The spectrum estimates of the set-ups.  which = 0: the rho hope_setup ends with for the CSR matrix as given (katz_rho_estimate: margin and cap
// applied).  which = 1: the c gemhip_lle ends with (lle_shift_estimate) -- the rows are l1-normalised here as gemhip_lle normalises them.
extern "C" int gemhip_test_hope_spectrum_estimate(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t which,
                                                  double *estimate_out)
{
    GEMHIP_REQUIRE(hook_csr_ok(n, nnz, row_ptr, col), "test_hope_spectrum_estimate: bad CSR arguments");
    GEMHIP_REQUIRE((which == 0 || which == 1) && estimate_out, "test_hope_spectrum_estimate: bad arguments");
    Hope H;
    std::vector<float> va(std::max<int64_t>(nnz, 1), 1.0f);
    if (which == 1) lle_edge_values(n, row_ptr, w, va.data());
    else if (w) std::copy(w, w + nnz, va.begin());
    upload_csr_w(H, n, nnz, row_ptr, col, va.data(), true);
    if (which == 1) H.mode = 2;
    const double est = which == 0 ? katz_rho_estimate(H, row_ptr, col, va.data()) : lle_shift_estimate(H);
    if (!H.err) *estimate_out = est;
    return H.err;
}
