// argarch_sim.cpp — the ARGARCH pass routines, ARModel's pair and the sample recursions of
// spark-timeseries_amd/csrc/model_pass.hpp on the CPU (TEST INFRASTRUCTURE): the loops k_model_fit<ArGarch>,
// k_model_effects<ArGarch>, k_ar_effects and k_garch_sample run per lane, for every row of a file.
// tests/test_argarch_ref.py compares the output bit for bit with tests/argarch_ref.py.
//
//   argarch_sim <mode> <in> <out>
//   in : int64 N, int64 T, int64 P, then N x T doubles (rows, row-major), then N x P doubles (parameters per row)
//   mode fit               P = 2 (c, phi of the AR stage); out: N x 3 doubles (omega, alpha, beta), N doubles (objective),
//                          N int32 status, N int32 n_eval, N int32 n_grad
//   mode remove | add      P = 5 (c, phi, omega, alpha, beta); out: N x T doubles
//   mode gsample | asample P = 3 | 5; rows = the normals; out: N x T doubles
//   mode arremove | aradd  P = 1 + p (c, phi_1 .. phi_p); out: N x T doubles
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../spark-timeseries_amd/csrc/model_pass.hpp"

using namespace sts::small;

static int run_fit(const std::vector<double> &rows, const std::vector<double> &par, int64_t N, int64_t T, FILE *out) {
    constexpr int K = ArGarch::K;
    std::vector<double> coef((size_t)N * K), obj((size_t)N);
    std::vector<int32_t> status((size_t)N), n_eval((size_t)N), n_grad((size_t)N);
    for (int64_t i = 0; i < N; ++i) {
        const double *row = rows.data() + (size_t)i * (size_t)T;
        SmallCG<K, ArGarch::kMinimize> m;
        double x0[K];
        ArGarch::initial_guess(x0);
        m.start(x0, 1e-6);
        while (!m.done()) {
            ArGarch::Pass ps;
            ps.begin(m.xreq(), &par[(size_t)i * ArGarch::A]);
            for (int t = 0; t < (int)T; ++t) ps.step(t, row[t]);
            double f, g[K];
            ps.end((int)T, &f, g);
            m.advance(f, g);
        }
        m.result(&coef[(size_t)i * K], &obj[(size_t)i]);
        status[(size_t)i] = m.status;
        n_eval[(size_t)i] = m.n_eval;
        n_grad[(size_t)i] = m.n_grad;
    }
    const size_t n = (size_t)N;
    if (fwrite(coef.data(), sizeof(double), n * K, out) != n * K) return 3;
    if (fwrite(obj.data(), sizeof(double), n, out) != n) return 3;
    if (fwrite(status.data(), sizeof(int32_t), n, out) != n) return 3;
    if (fwrite(n_eval.data(), sizeof(int32_t), n, out) != n) return 3;
    if (fwrite(n_grad.data(), sizeof(int32_t), n, out) != n) return 3;
    return 0;
}

template <class Fx>
static void stream_row(Fx &fx, const double *row, double *o, int64_t T) {
    for (int t = 0; t < (int)T; ++t) o[t] = fx.step(t, row[t]);
}

template <class Fx>
static int run_fx(const std::vector<double> &rows, const std::vector<double> &par, int64_t N, int64_t T, int64_t P,
                  FILE *out) {
    std::vector<double> o((size_t)N * (size_t)T);
    for (int64_t i = 0; i < N; ++i) {
        Fx fx;
        fx.begin(&par[(size_t)i * (size_t)P]);
        stream_row(fx, rows.data() + (size_t)i * (size_t)T, o.data() + (size_t)i * (size_t)T, T);
    }
    return fwrite(o.data(), sizeof(double), o.size(), out) == o.size() ? 0 : 3;
}

template <bool ADD>
static int run_ar(const std::vector<double> &rows, const std::vector<double> &par, int64_t N, int64_t T, int64_t P,
                  FILE *out) {
    const int p = (int)P - 1;
    std::vector<double> o((size_t)N * (size_t)T), hist((size_t)p);       // exactly p: the sanitizer sees any overrun
    for (int64_t i = 0; i < N; ++i) {
        ArFx<ADD> fx;
        fx.begin(&par[(size_t)i * (size_t)P], p, hist.data());
        stream_row(fx, rows.data() + (size_t)i * (size_t)T, o.data() + (size_t)i * (size_t)T, T);
    }
    return fwrite(o.data(), sizeof(double), o.size(), out) == o.size() ? 0 : 3;
}

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s <fit|remove|add|gsample|asample|arremove|aradd> <in> <out>\n", argv[0]);
        return 2;
    }
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 2;
    int64_t hdr[3];
    if (fread(hdr, sizeof(int64_t), 3, in) != 3 || hdr[0] < 0 || hdr[1] < 1 || hdr[2] < 1) { fclose(in); return 2; }
    const int64_t N = hdr[0], T = hdr[1], P = hdr[2];
    std::vector<double> rows((size_t)N * (size_t)T), par((size_t)N * (size_t)P);
    if (fread(rows.data(), sizeof(double), rows.size(), in) != rows.size() ||
        fread(par.data(), sizeof(double), par.size(), in) != par.size()) { fclose(in); return 2; }
    fclose(in);
    const char *mode = argv[1];
    const bool ar = !strcmp(mode, "arremove") || !strcmp(mode, "aradd");
    const int64_t want = !strcmp(mode, "fit") ? 2 : !strcmp(mode, "gsample") ? 3 : 5;
    if (ar ? (P < 2 || P > 1 + kArMaxP) : P != want) return 2;
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    int rc;
    if (!strcmp(mode, "fit")) rc = run_fit(rows, par, N, T, out);
    else if (!strcmp(mode, "remove")) rc = run_fx<ArGarch::Fx<false>>(rows, par, N, T, P, out);
    else if (!strcmp(mode, "add")) rc = run_fx<ArGarch::Fx<true>>(rows, par, N, T, P, out);
    else if (!strcmp(mode, "gsample")) rc = run_fx<GarchSample<false>>(rows, par, N, T, P, out);
    else if (!strcmp(mode, "asample")) rc = run_fx<GarchSample<true>>(rows, par, N, T, P, out);
    else if (!strcmp(mode, "arremove")) rc = run_ar<false>(rows, par, N, T, P, out);
    else if (!strcmp(mode, "aradd")) rc = run_ar<true>(rows, par, N, T, P, out);
    else rc = 2;
    fclose(out);
    return rc;
}
