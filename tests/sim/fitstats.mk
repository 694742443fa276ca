# Host build of the runtime's stats functions (fit_stats.hpp: counter names, the word-to-field table, the flops formula,
# fit / search / summed stats) against the bodies they replaced, as a stand-alone program (test infrastructure):
# make -f fitstats.mk [fitstats | fitstats_san]
# fitstats_san: the same under AddressSanitizer + UBSan (host code only, run on its own).
CXX     ?= g++
FSHDRS  := ../../spark-timeseries_amd/csrc/fit_stats.hpp ../../include/sparkts_arima.h
FSFLAGS := -O2 -std=c++17 -ffp-contract=off -Wall

fitstats: _build/fitstats_sim
fitstats_san: _build/fitstats_sim_san

_build/fitstats_sim: fitstats_sim.cpp $(FSHDRS)
	@mkdir -p _build
	$(CXX) $(FSFLAGS) -o $@ fitstats_sim.cpp

_build/fitstats_sim_san: fitstats_sim.cpp $(FSHDRS)
	@mkdir -p _build
	$(CXX) $(FSFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ fitstats_sim.cpp

.PHONY: fitstats fitstats_san
