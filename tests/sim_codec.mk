# What the CPU builds of the two codec libraries share (test infrastructure; see sim_codec.h): the decoder and the compressor of the
# gfx950 kernels, lane for lane on host memory.  The Makefile that includes this sets NAME and HDR (the headers of its core).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -Wall -Wextra -fPIC
SRC = brc_$(NAME)_sim.cpp
DEP = $(SRC) $(HDR) ../sim_codec.h
all: libbrc_$(NAME)_sim.so
libbrc_$(NAME)_sim.so: $(DEP)
	$(CXX) $(CXXFLAGS) -shared $(SRC) -o $@ -pthread
# the same library and a driver ($(NAME)_check.cpp says who feeds it) with the host sanitizers: every read outside a member's input and
# every write outside its slot is a report
asan: $(NAME)_check_asan
$(NAME)_check_asan: $(NAME)_check.cpp $(DEP)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=all -fno-omit-frame-pointer $(NAME)_check.cpp $(SRC) -o $@ -pthread
clean::
	rm -f libbrc_$(NAME)_sim.so $(NAME)_check_asan
