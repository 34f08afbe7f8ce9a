# TEST INFRASTRUCTURE: the emulator library of Makefile plus ILU(k) (kk_spiluk.hip) and the sparse triangular solve it takes its level
# sets from (kk_sptrsv.hip), for tests/test_emu_spiluk.py.  Makefile itself stays as it is; its objects are shared.
include Makefile
kk_spiluk.emu.o: $(CSRC)/kk_spiluk_fill.h
kk_sptrsv.emu.o kk_spiluk.emu.o: $(CSRC)/kk_levels.h
libkkamd_emu_spiluk.so: $(OBJS) kk_sptrsv.emu.o kk_spiluk.emu.o
	$(CXX) -shared -o $@ $(OBJS) kk_sptrsv.emu.o kk_spiluk.emu.o
# the host side of the symbolic phase alone, under the host sanitizers
spiluk_fill_check: spiluk_fill_check.cpp $(CSRC)/kk_spiluk_fill.h
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) spiluk_fill_check.cpp -o $@
