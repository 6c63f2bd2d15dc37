// liboicc_hip, host side: the options of the two problem objects as plain structs of doubles.  oicc_options.def (oicc_problem) and
// oicc_ba_options.def (oicc_ba) are the only lists of option names; each is expanded twice below, into the members with their
// defaults and into the table the setters, getters and oicc_debug_option_table look names up in.  A reader is a member access:
// a misspelt name does not compile, a read writes nothing (two threads may read), and only what a .def lists is an option.
#pragma once
#include <cstring>

namespace oicc {

struct OiccOptions {
#define OICC_OPT(name, value) double name = value;
#include "oicc_options.def"
#undef OICC_OPT
};

struct OiccBaOptions {
#define OICC_OPT(name, value) double name = value;
#include "oicc_ba_options.def"
#undef OICC_OPT
};

template <class T> struct OptionEntry { const char* name; double default_value; double T::*member; };

inline const OptionEntry<OiccOptions> kOptionTable[] = {
#define OICC_OPT(name, value) {#name, value, &OiccOptions::name},
#include "oicc_options.def"
#undef OICC_OPT
};

inline const OptionEntry<OiccBaOptions> kBaOptionTable[] = {
#define OICC_OPT(name, value) {#name, value, &OiccBaOptions::name},
#include "oicc_ba_options.def"
#undef OICC_OPT
};

// the member of that name; nullptr: there is no such option
template <class T, size_t N> double* find_option(T& opt, const OptionEntry<T> (&table)[N], const char* name) {
  for (const OptionEntry<T>& e : table) if (!std::strcmp(e.name, name)) return &(opt.*e.member);
  return nullptr;
}
inline double* find_option(OiccOptions& opt, const char* name) { return find_option(opt, kOptionTable, name); }
inline double* find_option(OiccBaOptions& opt, const char* name) { return find_option(opt, kBaOptionTable, name); }

}  // namespace oicc
