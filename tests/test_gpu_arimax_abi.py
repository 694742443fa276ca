"""The argument contract of the ARIMAX entry points (include/sparkts_arima.h): padded rows and strides on a caller's
stream with sentinels behind every output, nullable counters, overlapping buffers, N == 0 and the refused arguments."""
import numpy as np
import pytest

import arimax_cases as C
import arimax_ref as AX
import sparkts_amd._lib as L
from test_gpu_diag import _same

pytestmark = pytest.mark.gpu

SENT = -7.0


def _padded(rows, ld):
    h = np.full((rows.shape[0], ld), SENT)
    h[:, :rows.shape[1]] = rows
    return h


def test_device_fit_on_a_caller_stream(engine):
    import torch
    p, d, q, Lx, orig, icpt, T, k = C.CONFIGS["b"]
    N, ld, xs = 70, T + 3, k * T + 5
    y, x = (a[:N] for a in C.batch("b"))
    ref = C.batch_ref("b", engine.get_option("smear"))
    Kp = AX.num_coef(k, p, q, Lx, orig)
    yh = _padded(y, ld)
    xh = _padded(x.transpose(0, 2, 1).reshape(N, k * T), xs)
    yd, xd = torch.from_numpy(yh).cuda(), torch.from_numpy(xh).cuda()
    coef = [torch.full((N * Kp + 8,), SENT, dtype=torch.float64, device="cuda") for _ in range(2)]
    ll = [torch.full((N + 8,), SENT, dtype=torch.float64, device="cuda") for _ in range(2)]
    ints = [torch.full((N + 8,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream
    args = (yd.data_ptr(), N, T, ld, xd.data_ptr(), xs, k, p, d, q, Lx, orig, icpt)
    engine.arimax_fit_device(*args, coef[0].data_ptr(), ll[0].data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(),
                             ints[2].data_ptr(), stream=s, blocking=False)
    engine.arimax_fit_device(*args, coef[1].data_ptr(), ll[1].data_ptr(), ints[3].data_ptr(), stream=s)   # no counters
    assert np.array_equal(yd.cpu().numpy(), yh) and np.array_equal(xd.cpu().numpy(), xh)
    st0, ne, ng, st1 = (a.cpu().numpy() for a in ints)
    for a in (st0, ne, ng, st1):
        assert np.all(a[N:] == -7), "written past an output"
    for c, l_ in zip(coef, ll):
        c, l_ = c.cpu().numpy(), l_.cpu().numpy()
        assert np.all(c[N * Kp:] == SENT) and np.all(l_[N:] == SENT), "written past an output"
        assert _same(c[:N * Kp].reshape(N, Kp), ref["coef"][:N]) and _same(l_[:N], ref["ll"][:N])
    assert np.array_equal(st0[:N], ref["status"][:N]) and np.array_equal(st1[:N], ref["status"][:N])
    assert np.array_equal(ne[:N], ref["n_eval"][:N]) and np.array_equal(ng[:N], ref["n_grad"][:N])
    # user_init on the device: the restated start gives the restated fit
    init = torch.from_numpy(np.ascontiguousarray(ref["init"][:N])).cuda()
    engine.arimax_fit_device(*args, coef[1].data_ptr(), ll[1].data_ptr(), ints[3].data_ptr(),
                             d_user_init=init.data_ptr(), stream=s)
    ok = ref["status"][:N] == AX.ST_OK
    assert _same(coef[1].cpu().numpy()[:N * Kp].reshape(N, Kp)[ok], ref["coef"][:N][ok])


def test_device_forecast_on_a_caller_stream(engine):
    import torch
    shape = next(s for s in C.forecast_shapes() if s[5] == 3 and s[2] == 1 and s[3][1] > 0)
    T, rule, d, (orig, Lx, icpt), (p, q), k = shape
    y, x, coef, ref = C.forecast_case(shape)
    N, nF = y.shape[0], x.shape[1]
    ld, ld_out, xs = T + 5, T + 2, k * nF + 3
    yh = _padded(y, ld)
    xh = _padded(x.transpose(0, 2, 1).reshape(N, k * nF), xs)
    yd, xd, cd = torch.from_numpy(yh).cuda(), torch.from_numpy(xh).cuda(), torch.from_numpy(coef).cuda()
    out = torch.full((N, ld_out), SENT, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    engine.arimax_forecast_device(yd.data_ptr(), N, T, ld, xd.data_ptr(), xs, k, nF, p, d, q, Lx, orig, icpt,
                                  cd.data_ptr(), out.data_ptr(), ld_out, stream=stream.cuda_stream)
    o = out.cpu().numpy()
    assert np.all(o[:, T:] == SENT) and _same(o[:, :T], ref)
    assert _same(yd.cpu().numpy(), yh) and _same(xd.cpu().numpy(), xh)      # (the ignored columns hold NaNs)
    # a shared matrix: series 4's, for everyone
    engine.arimax_forecast_device(yd.data_ptr(), N, T, ld, xd.data_ptr() + 4 * xs * 8, 0, k, nF, p, d, q, Lx, orig,
                                  icpt, cd.data_ptr(), out.data_ptr(), ld_out, stream=stream.cuda_stream)
    want = AX.arimax_forecast_batch(y, C.x_columns(x[4]), p, d, q, Lx, orig, icpt, coef)
    assert _same(out.cpu().numpy()[:, :T], want)


def test_refused_arguments(engine):
    import torch
    N, k, T, Kp = 8, 2, 24, 7                             # (1, 0, 1), L = 1 with the original columns
    sd = torch.zeros((N, T), dtype=torch.float64, device="cuda")
    xd = torch.zeros((k, T), dtype=torch.float64, device="cuda")
    out = torch.zeros((N * 16,), dtype=torch.float64, device="cuda")
    ints = torch.zeros((3 * N,), dtype=torch.int32, device="cuda")
    o, i = out.data_ptr(), ints.data_ptr()

    def fit(coef=o, ll=o + 8 * Kp * N, status=i, n_eval=i + 4 * N, n_grad=i + 8 * N, ld=T, xs=0, kx=k, p=1, d=0, q=1,
            Lx=1, n=N, series=sd.data_ptr(), xreg=xd.data_ptr(), init=None):
        return engine.L.arima_arimax_fit_batch_device(engine.h, series, n, T, ld, xreg, xs, kx, p, d, q, Lx, 1, 1, init,
                                                      coef, ll, status, n_eval, n_grad, None)

    assert fit() == L.ARIMA_OK
    assert fit(n_eval=None, n_grad=None) == L.ARIMA_OK
    assert fit(n=0, coef=None, ll=None, status=None) == L.ARIMA_OK          # N == 0: nothing is looked at
    assert fit(coef=sd.data_ptr()) == L.ARIMA_E_INVALID_ARG                 # coef_out over the series
    assert fit(ll=xd.data_ptr()) == L.ARIMA_E_INVALID_ARG                   # ll_out over the regressors
    assert fit(ll=o + 8) == L.ARIMA_E_INVALID_ARG                           # ll_out inside coef_out
    assert fit(n_eval=i + 4) == L.ARIMA_E_INVALID_ARG                       # n_eval_out inside status_out
    assert fit(init=o) == L.ARIMA_E_INVALID_ARG                             # coef_out over user_init
    assert fit(ld=T - 1) == L.ARIMA_E_INVALID_ARG
    assert fit(xs=k * T - 1) == L.ARIMA_E_INVALID_ARG                       # a stride in (0, k T)
    assert fit(kx=0) == L.ARIMA_E_INVALID_ARG and fit(kx=-1) == L.ARIMA_E_INVALID_ARG
    for kw in (dict(p=-1), dict(d=-1), dict(q=-1), dict(Lx=-1), dict(n=-1)):
        assert fit(**kw) == L.ARIMA_E_INVALID_ARG, kw
    for kw in (dict(coef=None), dict(ll=None), dict(status=None), dict(series=None), dict(xreg=None)):
        assert fit(**kw) == L.ARIMA_E_INVALID_ARG, kw
    assert fit(p=21) == L.ARIMA_E_UNSUPPORTED and fit(d=17) == L.ARIMA_E_UNSUPPORTED
    engine.synchronize()
    assert engine.L.arima_arimax_num_coef(2, 1, 1, 1, 1) == Kp and engine.L.arima_arimax_num_coef(4, 0, 2, 1, 1) == 11
    assert engine.L.arima_arimax_num_coef(2, 2, 1, 1, 0) == 6 and engine.L.arima_arimax_num_coef(-1, 0, 0, 0, 1) < 0
    assert engine.arimax_fit(np.zeros((0, T)), np.zeros((T, k)), 1, 0, 1, 1)["coef"].shape == (0, Kp)
    # the host forecast refuses an output over its input
    y = np.ones((2, T))
    x = np.ones((k, 5))
    coef = np.full((2, Kp), 0.1)
    rc = engine.L.arima_arimax_forecast_batch(engine.h, L._ptr(y), 2, T, L._ptr(x), 0, k, 5, 1, 0, 1, 1, 1, 1,
                                              L._ptr(coef), L._ptr(y))
    assert rc == L.ARIMA_E_INVALID_ARG
