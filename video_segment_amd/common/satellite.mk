# The build of a library of its own beside libvsg_hip.so, included by render/, flow/ and resize/
# Makefile after they set NAME (the library is ../lib/lib$(NAME).so), OBJS and HDRS.  Compiled for
# gfx950 with hipcc.  -ffp-contract=off -fno-fast-math: each library has a model under tests/ that
# defines its arithmetic, every operation rounded on its own, and has to equal it bit for bit.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
FLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall \
        -Wno-unused-function -Wno-unused-result
OBJDIR = build
LIBDIR = ../lib

all: $(LIBDIR)/lib$(NAME).so

# a library newer than its sources is up to date even when the object files are gone
.SECONDARY: $(OBJS)

$(OBJDIR)/%.o: %.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(FLAGS) -c $< -o $@

$(OBJDIR)/%.o: %.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(FLAGS) -x hip -c $< -o $@

$(LIBDIR)/lib$(NAME).so: $(OBJS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib

clean:
	rm -rf $(OBJDIR) $(LIBDIR)/lib$(NAME).so
