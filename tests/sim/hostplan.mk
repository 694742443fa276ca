# Host build of the runtime's host-side planners (host_plan.hpp: chunk schedule, pinned-staging layout, par_memcpy,
# slice rows) as a stand-alone sweep program (test infrastructure): make -f hostplan.mk [hostplan | hostplan_san]
# hostplan_san: the same under AddressSanitizer + UBSan (host code only, run on its own).
CXX     ?= g++
HPHDRS  := ../../spark-timeseries_amd/csrc/host_plan.hpp
HPFLAGS := -O2 -std=c++17 -pthread -Wall

hostplan: _build/hostplan_sim
hostplan_san: _build/hostplan_sim_san

_build/hostplan_sim: hostplan_sim.cpp $(HPHDRS)
	@mkdir -p _build
	$(CXX) $(HPFLAGS) -o $@ hostplan_sim.cpp

_build/hostplan_sim_san: hostplan_sim.cpp $(HPHDRS)
	@mkdir -p _build
	$(CXX) $(HPFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ hostplan_sim.cpp

.PHONY: hostplan hostplan_san
