// What host/pipeline.cpp and libdpe_mvs.so provide in the library, for a stand-alone sanitizer program that links a
// few host sources only: the last error (g_msg, which the program reads in its failure messages) and a device that
// is not there.  Included once, by the program's own source; the device entries of the sources it links are its own.
#pragma once
#include <string>

#include "../../include/dpe_host.h"

static std::string g_msg;
namespace dpe_host { void set_last_error(const std::string& m) { g_msg = m; } }
extern "C" const char* dpe_pipeline_last_error(void) { return g_msg.c_str(); }
extern "C" DpeContext* dpe_create(int) { return nullptr; }
extern "C" void dpe_destroy(DpeContext*) {}
extern "C" const char* dpe_last_error(void) { return "no device in this program"; }
