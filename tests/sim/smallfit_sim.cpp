// smallfit_sim.cpp — the small-model fit's optimizer state machine (spark-timeseries_amd/csrc/cg_small.hpp) and pass
// routines (model_pass.hpp) on the CPU (TEST INFRASTRUCTURE): the loop k_model_fit runs per lane -- post a point, one
// joint objective + gradient pass over the row, advance -- for every row of a file. tests/test_smallfit_ref.py compares
// the output bit for bit with tests/smallfit_ref.py.
//
//   smallfit_sim <ewma|garch> <in> <out>
//   in : int64 N, int64 T, then N x T doubles (row-major)
//   out: N x K doubles (parameters), N doubles (objective), N int32 status, N int32 n_eval, N int32 n_grad
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../spark-timeseries_amd/csrc/model_pass.hpp"

using namespace sts::small;

template <class Model>
static int run(const std::vector<double> &rows, int64_t N, int64_t T, FILE *out) {
    constexpr int K = Model::K;
    std::vector<double> coef((size_t)N * K), obj((size_t)N);
    std::vector<int32_t> status((size_t)N), n_eval((size_t)N), n_grad((size_t)N);
    for (int64_t i = 0; i < N; ++i) {
        const double *row = rows.data() + (size_t)i * (size_t)T;
        SmallCG<K, Model::kMinimize> m;
        double x0[K];
        Model::initial_guess(x0);
        m.start(x0, 1e-6);
        while (!m.done()) {
            typename Model::Pass ps;
            ps.begin(m.xreq());
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
    size_t n = (size_t)N;
    if (fwrite(coef.data(), sizeof(double), n * K, out) != n * K) return 3;
    if (fwrite(obj.data(), sizeof(double), n, out) != n) return 3;
    if (fwrite(status.data(), sizeof(int32_t), n, out) != n) return 3;
    if (fwrite(n_eval.data(), sizeof(int32_t), n, out) != n) return 3;
    if (fwrite(n_grad.data(), sizeof(int32_t), n, out) != n) return 3;
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s <ewma|garch> <in> <out>\n", argv[0]);
        return 2;
    }
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 2;
    int64_t hdr[2];
    if (fread(hdr, sizeof(int64_t), 2, in) != 2 || hdr[0] < 0 || hdr[1] < 1) { fclose(in); return 2; }
    const int64_t N = hdr[0], T = hdr[1];
    std::vector<double> rows((size_t)N * (size_t)T);
    if (fread(rows.data(), sizeof(double), rows.size(), in) != rows.size()) { fclose(in); return 2; }
    fclose(in);
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    int rc;
    if (!strcmp(argv[1], "ewma")) rc = run<Ewma>(rows, N, T, out);
    else if (!strcmp(argv[1], "garch")) rc = run<Garch>(rows, N, T, out);
    else rc = 2;
    fclose(out);
    return rc;
}
