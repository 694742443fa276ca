/*
 * sparkts_arima_jni.c — JNI shim between the Scala facade (ArimaMI355X.scala, this directory's ../src) and the
 * C ABI of the MI355X engine (include/sparkts_arima.h). It only forwards: direct NIO buffers are passed through as
 * plain pointers (no copies across JNI), return codes are returned unchanged. Build (needs a JDK):
 *     make -C integration/jvm/native JAVA_HOME=/path/to/jdk
 * The JVM method owner is the Scala object `ArimaMI355XNative`, whose JVM class is `ArimaMI355XNative$`
 * (hence `_00024` in the symbol names).
 *
 * Replaces, per call: ARIMA.fitModel over a bucket of equal-length series (ARIMA.scala:79-116),
 * ARIMAModel.forecast (ARIMA.scala:696-764), removeTimeDependentEffects / addTimeDependentEffects (ARIMA.scala:629-667),
 * the residual diagnostics autocorr / dwtest / lbtest (UnivariateTimeSeries.scala:70-96,
 * TimeSeriesStatisticalTests.scala:251-262, :298-307) and the order-search grid (ARIMA.scala:280-375, 826-830).
 */
#include <jni.h>
#include <stdint.h>

#include "sparkts_arima.h"

#define BUF(env, b) ((b) ? (*(env))->GetDirectBufferAddress((env), (b)) : NULL)
#define JNI_FN(name) Java_com_cloudera_sparkts_models_ArimaMI355XNative_00024_##name

JNIEXPORT jlong JNICALL JNI_FN(create)(JNIEnv *env, jobject self, jint device) {
    (void)env; (void)self;
    arima_handle *h = NULL;
    return arima_create(device, &h) == ARIMA_OK ? (jlong)(intptr_t)h : 0;
}

JNIEXPORT jint JNICALL JNI_FN(destroy)(JNIEnv *env, jobject self, jlong h) {
    (void)env; (void)self;
    return arima_destroy((arima_handle *)(intptr_t)h);
}

JNIEXPORT jstring JNICALL JNI_FN(lastError)(JNIEnv *env, jobject self, jlong h) {
    (void)self;
    return (*env)->NewStringUTF(env, arima_last_error((const arima_handle *)(intptr_t)h));
}

JNIEXPORT jint JNICALL JNI_FN(setOption)(JNIEnv *env, jobject self, jlong h, jstring name, jlong value) {
    (void)self;
    const char *s = (*env)->GetStringUTFChars(env, name, NULL);
    const int rc = arima_set_option((arima_handle *)(intptr_t)h, s, value);
    (*env)->ReleaseStringUTFChars(env, name, s);
    return rc;
}

/* arima_fit_batch: series N x T (DoubleBuffer), userInit N x k or null, outputs coef N x k, ll N, status N,
 * nEval / nGrad / flags N or null */
JNIEXPORT jint JNICALL JNI_FN(fitBatch)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n, jint t,
                                        jint p, jint d, jint q, jboolean intercept, jint method, jobject userInit,
                                        jobject coef, jobject ll, jobject status, jobject nEval, jobject nGrad,
                                        jobject flags) {
    (void)self;
    return arima_fit_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t, p, d, q,
                           intercept ? 1 : 0, method, (const double *)BUF(env, userInit), (double *)BUF(env, coef),
                           (double *)BUF(env, ll), (int32_t *)BUF(env, status), (int32_t *)BUF(env, nEval),
                           (int32_t *)BUF(env, nGrad), (uint8_t *)BUF(env, flags));
}

/* arima_forecast_batch: series N x T, coef N x k, out N x (T + nFuture) */
JNIEXPORT jint JNICALL JNI_FN(forecastBatch)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n, jint t,
                                             jint p, jint d, jint q, jboolean intercept, jobject coef,
                                             jint nFuture, jobject out) {
    (void)self;
    return arima_forecast_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t, p, d, q,
                                intercept ? 1 : 0, (const double *)BUF(env, coef), nFuture,
                                (double *)BUF(env, out));
}

/* arima_remove_effects_batch / arima_add_effects_batch (ARIMAModel.removeTimeDependentEffects, ARIMA.scala:629-644;
 * addTimeDependentEffects, :655-667): series / noise N x T, coef N x k, out N x T (out may be the input buffer) */
JNIEXPORT jint JNICALL JNI_FN(removeEffectsBatch)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n, jint t,
                                                  jint p, jint d, jint q, jboolean intercept, jobject coef,
                                                  jobject out) {
    (void)self;
    return arima_remove_effects_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t, p, d, q,
                                      intercept ? 1 : 0, (const double *)BUF(env, coef), (double *)BUF(env, out));
}

JNIEXPORT jint JNICALL JNI_FN(addEffectsBatch)(JNIEnv *env, jobject self, jlong h, jobject noise, jlong n, jint t,
                                               jint p, jint d, jint q, jboolean intercept, jobject coef,
                                               jobject out) {
    (void)self;
    return arima_add_effects_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, noise), n, t, p, d, q,
                                   intercept ? 1 : 0, (const double *)BUF(env, coef), (double *)BUF(env, out));
}

/* arima_diagnostics_batch: rows N x T; acf N x maxLag, dw N, lbStat N, lbPvalue N -- any of them may be null */
JNIEXPORT jint JNICALL JNI_FN(diagnosticsBatch)(JNIEnv *env, jobject self, jlong h, jobject rows, jlong n, jint t,
                                                jint maxLag, jobject acf, jobject dw, jobject lbStat,
                                                jobject lbPvalue) {
    (void)self;
    return arima_diagnostics_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, rows), n, t, maxLag,
                                   (double *)BUF(env, acf), (double *)BUF(env, dw), (double *)BUF(env, lbStat),
                                   (double *)BUF(env, lbPvalue));
}

/* arima_residual_diagnostics_batch: the same over the residuals of series N x T under the models coef N x k; the
 * residuals stay on the device */
JNIEXPORT jint JNICALL JNI_FN(residualDiagnosticsBatch)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n,
                                                        jint t, jint p, jint d, jint q, jboolean intercept,
                                                        jobject coef, jint maxLag, jobject acf, jobject dw,
                                                        jobject lbStat, jobject lbPvalue) {
    (void)self;
    return arima_residual_diagnostics_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t, p, d,
                                            q, intercept ? 1 : 0, (const double *)BUF(env, coef), maxLag,
                                            (double *)BUF(env, acf), (double *)BUF(env, dw),
                                            (double *)BUF(env, lbStat), (double *)BUF(env, lbPvalue));
}

/* arima_order_search_batch: series N x T, order N x 4, coef N x 11, aic N */
JNIEXPORT jint JNICALL JNI_FN(orderSearch)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n, jint t,
                                           jint maxP, jint maxD, jint maxQ, jint interceptMode, jint method,
                                           jobject order, jobject coef, jobject aic) {
    (void)self;
    return arima_order_search_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t, maxP,
                                    maxD, maxQ, interceptMode, method, (int32_t *)BUF(env, order),
                                    (double *)BUF(env, coef), (double *)BUF(env, aic));
}

/* arima_autofit_batch (ARIMA.autoFit, ARIMA.scala:280-375): series N x T, order N x 4, coef N x 11, aic / status /
 * n_fits N */
JNIEXPORT jint JNICALL JNI_FN(autoFit)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n, jint t, jint maxP,
                                       jint maxD, jint maxQ, jobject order, jobject coef, jobject aic, jobject status,
                                       jobject nFits) {
    (void)self;
    return arima_autofit_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t, maxP, maxD,
                               maxQ, (int32_t *)BUF(env, order), (double *)BUF(env, coef), (double *)BUF(env, aic),
                               (int32_t *)BUF(env, status), (int32_t *)BUF(env, nFits));
}

/* arima_ewma_fit_batch (EWMA.fitModel, EWMA.scala:45-69): series N x T; smoothing N, sse N, status N, nEval / nGrad N
 * or null */
JNIEXPORT jint JNICALL JNI_FN(ewmaFitBatch)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n, jint t,
                                            jobject smoothing, jobject sse, jobject status, jobject nEval,
                                            jobject nGrad) {
    (void)self;
    return arima_ewma_fit_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t,
                                (double *)BUF(env, smoothing), (double *)BUF(env, sse), (int32_t *)BUF(env, status),
                                (int32_t *)BUF(env, nEval), (int32_t *)BUF(env, nGrad));
}

/* arima_garch_fit_batch (GARCH.fitModel, GARCH.scala:33-53): series N x T; coef N x 3 (omega, alpha, beta), ll N,
 * status N, nEval / nGrad N or null */
JNIEXPORT jint JNICALL JNI_FN(garchFitBatch)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n, jint t,
                                             jobject coef, jobject ll, jobject status, jobject nEval, jobject nGrad) {
    (void)self;
    return arima_garch_fit_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t,
                                 (double *)BUF(env, coef), (double *)BUF(env, ll), (int32_t *)BUF(env, status),
                                 (int32_t *)BUF(env, nEval), (int32_t *)BUF(env, nGrad));
}

/* The TimeSeriesModel pairs of EWMAModel (EWMA.scala:125-143; smoothing N) and GARCHModel (GARCH.scala:131-162;
 * coef N x 3): series N x T, out N x T (out may not overlap an input) */
#define MODEL_EFFECTS_FN(jname, cname)                                                                             \
    JNIEXPORT jint JNICALL JNI_FN(jname)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n, jint t,      \
                                         jobject params, jobject out) {                                            \
        (void)self;                                                                                                \
        return cname((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t,                          \
                     (const double *)BUF(env, params), (double *)BUF(env, out));                                   \
    }
MODEL_EFFECTS_FN(ewmaRemoveEffectsBatch, arima_ewma_remove_effects_batch)
MODEL_EFFECTS_FN(ewmaAddEffectsBatch, arima_ewma_add_effects_batch)
MODEL_EFFECTS_FN(garchRemoveEffectsBatch, arima_garch_remove_effects_batch)
MODEL_EFFECTS_FN(garchAddEffectsBatch, arima_garch_add_effects_batch)

/* arima_argarch_fit_batch (ARGARCH.fitModel, GARCH.scala:63-69): series N x T; coef N x 5 (c, phi, omega, alpha,
 * beta), ll N, status N, nEval / nGrad N or null */
JNIEXPORT jint JNICALL JNI_FN(argarchFitBatch)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n, jint t,
                                               jobject coef, jobject ll, jobject status, jobject nEval, jobject nGrad) {
    (void)self;
    return arima_argarch_fit_batch((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t,
                                   (double *)BUF(env, coef), (double *)BUF(env, ll), (int32_t *)BUF(env, status),
                                   (int32_t *)BUF(env, nEval), (int32_t *)BUF(env, nGrad));
}

/* ARGARCHModel's pair (GARCH.scala:205-236; coef N x 5) and GARCHModel.sample / ARGARCHModel.sample (:164-185,
 * :238-259) from the caller's gaussians z N x T (coef N x 3 / N x 5): out N x T (out may not overlap an input) */
MODEL_EFFECTS_FN(argarchRemoveEffectsBatch, arima_argarch_remove_effects_batch)
MODEL_EFFECTS_FN(argarchAddEffectsBatch, arima_argarch_add_effects_batch)
MODEL_EFFECTS_FN(garchSampleBatch, arima_garch_sample_batch)
MODEL_EFFECTS_FN(argarchSampleBatch, arima_argarch_sample_batch)

/* ARModel's pair (Autoregression.scala:60-90) at order p: series N x T, coef N x (1 + p) = (c, phi_1 .. phi_p) */
#define AR_EFFECTS_FN(jname, cname)                                                                                \
    JNIEXPORT jint JNICALL JNI_FN(jname)(JNIEnv *env, jobject self, jlong h, jobject series, jlong n, jint t,      \
                                         jint p, jobject coef, jobject out) {                                      \
        (void)self;                                                                                                \
        return cname((arima_handle *)(intptr_t)h, (const double *)BUF(env, series), n, t, p,                       \
                     (const double *)BUF(env, coef), (double *)BUF(env, out));                                     \
    }
AR_EFFECTS_FN(arRemoveEffectsBatch, arima_ar_remove_effects_batch)
AR_EFFECTS_FN(arAddEffectsBatch, arima_ar_add_effects_batch)
