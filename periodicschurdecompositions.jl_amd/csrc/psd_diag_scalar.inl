// psd_diag_scalar: the engine's scalar device routines, one call per lane (TEST PLUMBING, psd_mi355x.h).
// Included at the end of psd_engine.cpp (one translation unit), after psd_check_host.inl (psd_devbuf).
//
// The kernel only moves operands: every value it writes comes out of a routine as psd_platform.h, psd_scalar.h,
// psd_complex.h, psd_hess2.h, psd_zhess2.h and psd_chase3.h define it, compiled with the flags of the library it is
// built into.  Rows of 8 doubles per case; the slots of each op are listed at psd_diag_scalar_op in psd_mi355x.h.

PSD_KERNEL_B(64) psd_diag_scalar_kernel(int op, int ncases, const double* in, double* out) {
    PSD_PAR_ALL64(t) {
        const int cs_ = PSD_BLOCK_X * 64 + t;
        if (cs_ < ncases) {
            const double* a = in + (size_t)cs_ * 8;
            double o[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            switch (op) {
            case PSD_DS_RCP:
                o[0] = psd_rcp_fast(a[0]);
                break;
            case PSD_DS_SQRT_PAIR:
                psd_sqrt_pair_fast(a[0], o[0], o[1]);
                break;
            case PSD_DS_RSQRT2:
                psd_rsqrt2_fast(a[0], a[1], o[0], o[1]);
                break;
            case PSD_DS_REFL2:
            case PSD_DS_REFL2_LEAN: {
                double x0 = a[0], x1 = a[1];
                o[2] = (op == PSD_DS_REFL2) ? psd_refl2(x0, x1) : psd_refl2_lean(x0, x1);
                o[0] = x0;
                o[1] = x1;
                break;
            }
            case PSD_DS_REFL3:
            case PSD_DS_REFL3_LEAN: {
                double x0 = a[0], x1 = a[1], x2 = a[2];
                o[3] = (op == PSD_DS_REFL3) ? psd_refl3(x0, x1, x2) : psd_refl3_lean(x0, x1, x2);
                o[0] = x0;
                o[1] = x1;
                o[2] = x2;
                break;
            }
            case PSD_DS_REFL32_PAIR: {
                double x0 = a[0], x1 = a[1], x2 = a[2], y0 = a[3], y1 = a[4];
                psd_refl32_pair(x0, x1, x2, o[3], y0, y1, o[6]);
                o[0] = x0;
                o[1] = x1;
                o[2] = x2;
                o[4] = y0;
                o[5] = y1;
                break;
            }
            case PSD_DS_REFLECTOR_SMALL: {
                double x[3] = {a[1], a[2], a[3]};
                o[3] = psd_reflector_small(x, (a[0] == 3.0) ? 3 : 2);
                o[0] = x[0];
                o[1] = x[1];
                o[2] = (a[0] == 3.0) ? x[2] : 0.0;
                break;
            }
            case PSD_DS_H2_LARFG:
                psd_h2_larfg(a[0], a[1], o[0], o[1], o[2]);
                break;
            case PSD_DS_ZH2_LARFG: {
                psd_z tau, mult;
                psd_zh2_larfg(zmk(a[0], a[1]), a[2], tau, o[2], mult);
                o[0] = tau.re;
                o[1] = tau.im;
                o[3] = mult.re;
                o[4] = mult.im;
                break;
            }
            case PSD_DS_GIVENS:
                psd_givens(a[0], a[1], o[0], o[1], o[2]);
                break;
            case PSD_DS_ZGIVENS:
            case PSD_DS_ZGIVENS_LEAN: {
                psd_z sn, r;
                if (op == PSD_DS_ZGIVENS) psd_zgivens(zmk(a[0], a[1]), zmk(a[2], a[3]), o[0], sn, r);
                else psd_zgivens_lean(zmk(a[0], a[1]), zmk(a[2], a[3]), o[0], sn, r);
                o[1] = sn.re;
                o[2] = sn.im;
                o[3] = r.re;
                o[4] = r.im;
                break;
            }
            case PSD_DS_C3_SCALE: {
                // (e travels as a double; the clamp keeps the conversion defined, not the routines in range)
                const int e = (int)fmin(fmax(a[2], -4096.0), 4096.0);
                o[0] = (double)psd_c3_expo(a[0]);
                o[1] = psd_c3_ldexp(a[1], e);
                o[2] = psd_c3_beta(a[3], a[4], e);
                break;
            }
            default:
                break;
            }
            double* q = out + (size_t)cs_ * 8;
            for (int k = 0; k < 8; ++k) q[k] = o[k];
        }
    }
}

namespace {
int diag_scalar_run(psd_ctx* c, int op, int ncases, const double* in, double* out) {
    const size_t bytes = sizeof(double) * 8 * (size_t)ncases;
    psd_devbuf bin, bout;
    PSD_CHECK(bin.alloc(bytes));
    PSD_CHECK(bout.alloc(bytes));
    PSD_CHECK(psd_rt_h2d(bin.p, in, bytes, c->stream));
    PSD_LAUNCH(psd_diag_scalar_kernel, psd_dim3((ncases + 63) / 64), 64, 0, c->stream, op, ncases, (const double*)bin.d(),
               bout.d());
    PSD_CHECK(psd_rt_d2h(out, bout.p, bytes, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    return 0;
}
}  // namespace

extern "C" int psd_diag_scalar(psd_ctx* c, int op, int ncases, const double* in, double* out, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (!c) return *info = -1;
    if (op < 0 || op >= PSD_DS_NOPS) return *info = -2;
    if (ncases < 1) return *info = -3;
    if (!in) return *info = -4;
    if (!out) return *info = -5;
    return *info = diag_scalar_run(c, op, ncases, in, out);
}
