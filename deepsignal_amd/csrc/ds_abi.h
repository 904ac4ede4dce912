// ds_abi.h — the exception firewall of the C ABI (include/deepsignal_hip.h: no entry point throws). Host only, no HIP.
//
// Every extern "C" function that returns int or int64_t is a function-try-block,
//     int ds_x(ds_handle* h, ...) try { ... } catch (...) { return abi_error(h); }
// and abi_error is a one-line overload beside the entry points of each file: it names the object's error text (ds_handle::err
// or the thread's create error in ds_engine.cpp, ds_tsv::err in ds_io.cpp) and calls caught(). The void entries swallow,
// the const char* ones allocate nothing. tests/test_abi_firewall.py holds every definition to this form.
#pragma once
#include "../../include/deepsignal_hip.h"

#include <exception>
#include <new>
#include <string>

namespace ds_abi {

// the text of an error into *sink (null: the entry has none); an allocation that fails here leaves the code to speak alone
inline void put(std::string* sink, const char* text, const char* more = nullptr) noexcept
{
    if (!sink) return;
    try {
        sink->assign(text);
        if (more) sink->append(more);
    } catch (...) {
        sink->clear();
    }
}

// Called from a catch (...): the DS_ERR_* code of the exception in flight, its text to *sink.
inline int caught(std::string* sink) noexcept
{
    try {
        throw;
    } catch (const std::bad_alloc&) {
        put(sink, "out of host memory");
        return DS_ERR_NOMEM;
    } catch (const std::exception& e) {
        put(sink, "internal error: ", e.what());
    } catch (...) {
        put(sink, "internal error");
    }
    return DS_ERR_INVALID;
}

}  // namespace ds_abi
