# What the CPU builds of the side libraries share (test infrastructure; see sim_side.h): the per-lane functions of the gfx950 kernels,
# lane for lane on host memory.  The Makefile that includes this sets NAME and HDR (the headers of its core), and WARN where its core
# needs a warning switched off.  -ffp-contract=off as in the product: every average is one fp32 division.
CXX ?= g++
WARN ?= -Wall -Wextra
CXXFLAGS ?= -O2 -std=c++17 $(WARN) -fPIC -ffp-contract=off
SRC = brc_$(NAME)_sim.cpp
DEP = $(SRC) $(HDR) ../sim_side.h
all: libbrc_$(NAME)_sim.so
libbrc_$(NAME)_sim.so: $(DEP)
	$(CXX) $(CXXFLAGS) -shared $(SRC) -o $@
# the same code and a driver (tests/test_$(NAME).py feeds it its views and its calls) with the host sanitizers: every load outside a view
# or a list, and every store outside a scratch or a destination of exactly the contract's size, is a report
asan: $(NAME)_check_asan
$(NAME)_check_asan: $(NAME)_check.cpp $(DEP)
	$(CXX) -O1 -g -std=c++17 $(WARN) -ffp-contract=off -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=all -fno-omit-frame-pointer $(NAME)_check.cpp $(SRC) -o $@
clean:
	rm -f libbrc_$(NAME)_sim.so $(NAME)_check_asan
