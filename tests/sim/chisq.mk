# Host build of the chi-squared upper tail (arima_chisq.hpp, the header the device kernels include) as a stand-alone
# filter program (test infrastructure): make -f chisq.mk chisq. No contraction, as in the library's own build.
CXX     ?= g++
CQHDRS  := ../../spark-timeseries_amd/csrc/arima_chisq.hpp
CQFLAGS := -O2 -std=c++17 -ffp-contract=off -Wall

chisq: _build/chisq_host

_build/chisq_host: chisq_host.cpp $(CQHDRS)
	@mkdir -p _build
	$(CXX) $(CQFLAGS) -I../../spark-timeseries_amd/csrc -o $@ chisq_host.cpp

.PHONY: chisq
