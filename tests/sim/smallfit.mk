# Host build of the small models' optimizer state machine and pass routines (cg_small.hpp, model_pass.hpp) as a
# stand-alone program (test infrastructure): make -f smallfit.mk [smallfit | smallfit_san]
# smallfit_san: the same under AddressSanitizer + UBSan (host code only, run on its own).
CXX     ?= g++
SMHDRS  := ../../spark-timeseries_amd/csrc/cg_small.hpp ../../spark-timeseries_amd/csrc/model_pass.hpp ../../include/sparkts_arima.h
SMFLAGS := -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Wall

smallfit: _build/smallfit_sim
smallfit_san: _build/smallfit_sim_san

_build/smallfit_sim: smallfit_sim.cpp $(SMHDRS)
	@mkdir -p _build
	$(CXX) $(SMFLAGS) -o $@ smallfit_sim.cpp

_build/smallfit_sim_san: smallfit_sim.cpp $(SMHDRS)
	@mkdir -p _build
	$(CXX) $(SMFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ smallfit_sim.cpp

.PHONY: smallfit smallfit_san
