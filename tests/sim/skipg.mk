# Host build of the optimizer state machine with and without the skipped dead gradient (cg_lane.hpp, SKIPG) against
# the CPU restatement, as stand-alone programs (test infrastructure):
# make -f skipg.mk [skipg | skipg_san | _build/skipg_sim_maxeval<E> | _build/skipg_sim_maxiter<M>]
# skipg_san: the same under AddressSanitizer + UBSan (host code only, run on its own); maxeval<E> / maxiter<M>: the
# machine's MaxEval / MaxIter lowered to E / M, so that fits stop at the top of an iteration within milliseconds.
CXX     ?= g++
SGHDRS  := ../../spark-timeseries_amd/csrc/cg_lane.hpp ../../include/sparkts_arima.h ../../oracle/_build/libarima_oracle.so
SGFLAGS := -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-maybe-uninitialized
SGLINK  := -L../../oracle/_build -larima_oracle -Wl,-rpath,'$$ORIGIN/../../../oracle/_build'

skipg: _build/skipg_sim
skipg_san: _build/skipg_sim_san

_build/skipg_sim: skipg_sim.cpp $(SGHDRS)
	@mkdir -p _build
	$(CXX) $(SGFLAGS) -o $@ skipg_sim.cpp $(SGLINK)

_build/skipg_sim_san: skipg_sim.cpp $(SGHDRS)
	@mkdir -p _build
	$(CXX) $(SGFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ skipg_sim.cpp $(SGLINK)

_build/skipg_sim_maxeval%: skipg_sim.cpp $(SGHDRS)
	@mkdir -p _build
	$(CXX) $(SGFLAGS) -DSTS_CG_MAX_EVAL=$* -o $@ skipg_sim.cpp $(SGLINK)

_build/skipg_sim_maxiter%: skipg_sim.cpp $(SGHDRS)
	@mkdir -p _build
	$(CXX) $(SGFLAGS) -DSTS_CG_MAX_ITER=$* -o $@ skipg_sim.cpp $(SGLINK)

.PHONY: skipg skipg_san
