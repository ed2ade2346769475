/*
 * pdehip_shim_poisson_fft.c — HOST implementation of pdehip_fft_inverse and pdehip_poisson_fft (include/pdehip.h).  TESTS ONLY.
 *
 * An addition to the host shim (pdehip_shim.c, see the notice there): tests/poisson_fft_shimlib.py links this file with the shim's objects
 * into tests/shim/_build/libpdehip_shim_poisson_fft.so, so that `method="fft"` of pde_hip/poisson.py runs through the REAL py-pde without
 * a GPU, and so that the device kernels (csrc/pdehip_fft.hip, csrc/pdehip_fftsolve.hip) have a serial statement of their arithmetic to
 * be compared with bit by bit.  The product never builds or loads it.
 *
 * The forward half (twiddle, fft_line, forward_one and the three entry points that go with them) is that of pdehip_shim_spectrum.c,
 * included as it stands.  What is shared with the device code is the tables, the butterfly, the mirror rule and the division: no tiles,
 * no LDS, no waves; the four sums of the test are added cell by cell in C order.
 */
#include "pdehip_shim_spectrum.c"

/* the eigenvalue of -d^2/dx^2 on a periodic axis of n cells, mode m (the same lines: csrc/pdehip_fftsolve.hip) */
static double lap_eigenvalue(long m, long n, double scale)
{
    const long mm = m < n - m ? m : n - m;
    const double s = sin(3.14159265358979323846 * (double)mm / (double)n);
    return (4.0 * (s * s)) * scale;
}

/* the half spectrum (n0, n1, nh) of one component back into the interior cells of a full array; `spec` is consumed */
static int inverse_one(const rows_t *r, cplx_t *spec, void *out)
{
    const long n0 = r->n[0], n1 = r->n[1], n2 = r->n[2], nh = n2 / 2 + 1;
    long longest = n2 > n1 ? n2 : n1;
    if (n0 > longest) longest = n0;
    cplx_t *tw = (cplx_t *)malloc(sizeof(cplx_t) * (size_t)(longest / 2 + 1));
    cplx_t *line = (cplx_t *)malloc(sizeof(cplx_t) * (size_t)longest);
    cplx_t *work = (cplx_t *)malloc(sizeof(cplx_t) * (size_t)longest);
    if (!tw || !line || !work) { free(tw); free(line); free(work); return shim_set_error(3, "shim: fft: out of memory"); }
    if (n0 > 1) {
        for (long m = 0; m < n0 / 2; m++) { twiddle(m, n0, &tw[m].re, &tw[m].im); tw[m].im = -tw[m].im; }
        for (long w = 0; w < n1 * nh; w++) fft_line(spec + w, n1 * nh, log2_of(n0), tw, work);
    }
    if (n1 > 1) {
        for (long m = 0; m < n1 / 2; m++) { twiddle(m, n1, &tw[m].re, &tw[m].im); tw[m].im = -tw[m].im; }
        for (long i = 0; i < n0; i++)
            for (long k = 0; k < nh; k++) fft_line(spec + i * n1 * nh + k, nh, log2_of(n1), tw, work);
    }
    for (long m = 0; m < n2 / 2; m++) { twiddle(m, n2, &tw[m].re, &tw[m].im); tw[m].im = -tw[m].im; }
    const double inv_size = 1.0 / (double)(n0 * n1 * n2);
    for (long i = 0; i < n0; i++)
        for (long j = 0; j < n1; j++) {
            const cplx_t *row = spec + (i * n1 + j) * nh;
            for (long k = 0; k < n2; k++) {
                if (2 * k <= n2) line[k] = row[k];
                else { line[k].re = row[n2 - k].re; line[k].im = -row[n2 - k].im; }
            }
            fft_line(line, 1, log2_of(n2), tw, work);
            const long e = r->off + i * r->p[0] + j * r->p[1];
            for (long k = 0; k < n2; k++) {
                const double v = line[k].re * inv_size;
                if (r->f64) ((double *)out)[e + k] = v;
                else ((float *)out)[e + k] = (float)v;
            }
        }
    free(tw); free(line); free(work);
    return 0;
}

int pdehip_fft_inverse(const pdehip_grid_t *g, int ncomp, void *spectrum, void *out_full, void *stream)
{
    (void)stream;
    rows_t r;
    int rc = check_extents(g, &r);
    if (rc) return rc;
    if (!spectrum || !out_full) return shim_set_error(1, "shim: fft_inverse: NULL pointer");
    if (ncomp < 1 || ncomp > 64) return shim_set_error(1, "shim: fft_inverse: 1..64 components");
    if ((((uintptr_t)spectrum | (uintptr_t)out_full) & 15) != 0) return shim_set_error(1, "shim: fft_inverse: misaligned array");
    const long per = r.n[0] * r.n[1] * (r.n[2] / 2 + 1);
    const size_t esize = r.f64 ? 8 : 4;
    for (int c = 0; c < ncomp; c++) {
        rc = inverse_one(&r, (cplx_t *)spectrum + (size_t)c * per, (char *)out_full + (size_t)c * (size_t)r.pc * esize);
        if (rc) return rc;
    }
    return 0;
}

int pdehip_poisson_fft(const pdehip_grid_t *g, const void *rhs_full, void *out_full, pdehip_poisson_t *io, void *stream)
{
    (void)stream;
    rows_t rf, r64;
    int rc = check_extents(g, &rf);
    if (rc) return rc;
    if (!rhs_full || !out_full || !io) return shim_set_error(1, "shim: poisson_fft: NULL pointer");
    if ((((uintptr_t)rhs_full | (uintptr_t)out_full) & 15) != 0) return shim_set_error(1, "shim: poisson_fft: misaligned array");
    if (!(io->rtol >= 0) || !(io->atol >= 0)) return shim_set_error(1, "shim: poisson_fft: bad rtol / atol");
    pdehip_grid_t g64 = *g;
    g64.dtype = PDEHIP_F64;
    rc = make_rows(&g64, &r64);
    if (rc) return rc;
    const long n0 = rf.n[0], n1 = rf.n[1], n2 = rf.n[2], nh = n2 / 2 + 1, total = n0 * n1 * nh;
    const double size = (double)(n0 * n1 * n2);
    cplx_t *spec = (cplx_t *)malloc(sizeof(cplx_t) * (size_t)total);
    double *x = (double *)calloc((size_t)r64.pc + 2, sizeof(double)), *w = (double *)calloc((size_t)r64.pc + 2, sizeof(double));
    double *mu[3] = {(double *)malloc(sizeof(double) * (size_t)n0), (double *)malloc(sizeof(double) * (size_t)n1), (double *)malloc(sizeof(double) * (size_t)n2)};
    if (!spec || !x || !w || !mu[0] || !mu[1] || !mu[2]) {
        free(spec); free(x); free(w); free(mu[0]); free(mu[1]); free(mu[2]);
        return shim_set_error(3, "shim: poisson_fft: out of memory");
    }
    /* 1 / dx^2 as the Laplacian kernels use it (numpy's pow(dx, -2)); an absent axis has the scale 1 and the one entry 0 */
    for (int ax = 0; ax < 3; ax++) {
        const int a = ax - (3 - g->ndim);
        const double scale = a >= 0 ? pow(g->dx[a], -2.0) : 1.0;
        for (long m = 0; m < rf.n[ax]; m++) mu[ax][m] = lap_eigenvalue(m, rf.n[ax], scale);
    }
    rc = forward_one(&rf, rhs_full, spec);
    double mean = 0.0;
    if (!rc) {
        long t = 0;
        for (long i = 0; i < n0; i++)
            for (long j = 0; j < n1; j++)
                for (long k = 0; k < nh; k++, t++) {
                    if (t == 0) {
                        mean = spec[0].re / size;
                        spec[0].re = 0.0; spec[0].im = 0.0;
                        continue;
                    }
                    const double m = (mu[0][i] + mu[1][j]) + mu[2][k];
                    spec[t].re = (spec[t].re / m) * -1.0;
                    spec[t].im = (spec[t].im / m) * -1.0;
                }
        rc = inverse_one(&r64, spec, x);
    }
    if (!rc) {
        pdehip_bc_face_t faces[2 * PDEHIP_MAX_DIM];
        memset(faces, 0, sizeof(faces));
        for (int a = 0; a < g->ndim; a++)
            for (int side = 0; side < 2; side++) {
                pdehip_bc_face_t *f = &faces[2 * a + side];
                f->kind = PDEHIP_BC_ORDER1;
                f->index1 = side ? 0 : g->shape[a] - 1;
                f->factor1 = 1.0;
            }
        rc = pdehip_set_ghost_cells(&g64, 1, faces, x, NULL);
        if (!rc) rc = pdehip_laplace(&g64, x, w, PDEHIP_OUT_FULL, NULL);
    }
    if (!rc) {
        double cnt = 0, res = 0, resp = 0, fp = 0;
        for (long i = 0; i < n0; i++)
            for (long j = 0; j < n1; j++)
                for (long k = 0; k < n2; k++) {
                    const long e = r64.off + i * r64.p[0] + j * r64.p[1] + k, ef = rf.off + i * rf.p[0] + j * rf.p[1] + k;
                    const double f = rf.f64 ? ((const double *)rhs_full)[ef] : (double)((const float *)rhs_full)[ef];
                    const double d = w[e] - f;
                    if (!(fabs(d) <= 1e-5 + 1e-5 * fabs(f))) cnt = cnt + 1.0;
                    res = res + d * d;
                    const double gp = f - mean;
                    const double dp = w[e] - gp;
                    resp = resp + dp * dp;
                    fp = fp + gp * gp;
                    if (rf.f64) ((double *)out_full)[ef] = x[e];
                    else ((float *)out_full)[ef] = (float)x[e];
                }
        io->iterations = 0;
        io->singular = 1;
        io->reserved = 0;
        io->check_residual = sqrt(res);
        io->residual = sqrt(resp);
        io->rhs_norm = sqrt(fp);
        const double t = io->rtol * io->rhs_norm, tol = t > io->atol ? t : io->atol;
        if (!isfinite(cnt) || !isfinite(res) || !isfinite(resp) || !isfinite(fp)) io->status = 2;
        else if (cnt != 0) io->status = 4;
        else if (io->residual > tol) io->status = 1;
        else io->status = 0;
    }
    free(spec); free(x); free(w); free(mu[0]); free(mu[1]); free(mu[2]);
    return rc;
}
