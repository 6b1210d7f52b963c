// Environment switches of libfdx.
//
// The switches are the registry in fdx_env.cpp: 25 names, every one exercised by a test or a tool.  They are read ONCE - when the
// library first asks - and cached; fdx_env_reload() re-reads them (the tests change the environment between fits; a process that
// calls setenv while library threads run must not be raced by getenv at every call).  env("FDX_X") returns the cached value or
// NULL; a name that is not in the registry is a programming error (asserted by tests/test_host.py against the sources).
// env() and env_reload() may run concurrently from any threads, and a pointer env() returned stays valid for the life of the
// process, whatever is reloaded later.
#pragma once

namespace fdx {

const char* env(const char* name);
void env_reload();
// FDX_TRACE_HOST=1: host time since this thread's previous traced point (stderr, "scope: what"; scope may be NULL) - which calls
// the host spends its time in, and whether it keeps ahead of the device
void trace_host(const char* scope, const char* what);

}  // namespace fdx
