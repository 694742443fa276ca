# Host build of the ARGARCH pass routines, ARModel's pair and the sample recursions (model_pass.hpp over cg_small.hpp)
# as a stand-alone program (test infrastructure): make -f argarch.mk [argarch | argarch_san]
# argarch_san: the same under AddressSanitizer + UBSan (host code only, run on its own).
CXX     ?= g++
AGHDRS  := ../../spark-timeseries_amd/csrc/cg_small.hpp ../../spark-timeseries_amd/csrc/model_pass.hpp ../../include/sparkts_arima.h
AGFLAGS := -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Wall

argarch: _build/argarch_sim
argarch_san: _build/argarch_sim_san

_build/argarch_sim: argarch_sim.cpp $(AGHDRS)
	@mkdir -p _build
	$(CXX) $(AGFLAGS) -o $@ argarch_sim.cpp

_build/argarch_sim_san: argarch_sim.cpp $(AGHDRS)
	@mkdir -p _build
	$(CXX) $(AGFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ argarch_sim.cpp

.PHONY: argarch argarch_san
