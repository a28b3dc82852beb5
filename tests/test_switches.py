"""The native sources keep one code path per kernel: the only PV_* names a
preprocessor condition may test are the hooks, selectors and numeric
parameters listed here.  A variant that lost its A/B measurement lives as a
patch under tools/ab/, not as a compile-time switch in the product."""
import glob
import os
import re

from conftest import PKG, REPO

# name -> why a condition may test it
ALLOWED = {
    # qualifiers that a host build replaces or picks by compiler
    'PV_HD': 'host/device qualifier; host builds define it as plain inline',
    'PV_BN_CALL': 'out-of-line call qualifier of the BN254 layer (hipcc and host compilers differ)',
    # instrumentation that tools/hostcheck defines, empty in the product
    'PV_COUNT': 'operation counter hook of the host instrumentation build',
    'PV_CHECK_MUL': 'operand-bound check hook of fe_mul (host instrumentation build)',
    'PV_CHECK_SUB': 'operand-bound check hook of fe_sub / fe_sub4 (host instrumentation build)',
    'PV_CHECK_SQ': 'operand-bound check hook of fe_sq (host instrumentation build)',
    'PV_CHECK_SQ2X': 'operand-bound check hook of fe_sq2x (host instrumentation build)',
    'PV_BN_COUNT': 'operation counter hook of the BN254 host checker',
    'PV_BN_CHECK_MUL': 'column-sum bound check hook of the BN254 host checker',
    # plain C++ sums instead of inline asm: the branch every host build takes
    'PV_FE_NOASM': 'plain-sum field code; host builds take the same branch, tools/ubench/fe_salu.hip sets it',
    'PV_BN_NOASM': 'plain-sum BN254 code; host builds take the same branch',
    'PV_MADN_PLAIN': 'derived from PV_FE_NOASM / a host build (pv_madchains.h); the generated chains print it',
    'PV_BN_USE_ASM': 'derived from PV_BN_NOASM / a device build (pv_bn254.h)',
    # numeric launch / layout parameters with a single body
    'PV_CURVE_WAVES': 'waves per SIMD the curve kernels are compiled for',
    'PV_HASH_WAVES': 'waves per SIMD k_hash is compiled for',
    'PV_KEYS_WAVES': 'waves per SIMD k_keys is compiled for',
    'PV_HASH_CHUNK': 'fixed work-queue chunk size',
    'PV_HALF_LS': 'lane interleave of the half-size curve tables (a template argument)',
    'PV_CURVE_K': 'signatures per curve task, shared by pv_kernels.h and pv_verify_core.h',
    # defaults of run-time tuning values (pv_tuning)
    'PV_BLS_QUAD_MAX': 'default of pv_tuning.bls_quad_max',
    'PV_BLS_OCT_MAX': 'default of pv_tuning.bls_oct_max',
}

DIRECTIVE = re.compile(r'^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$')
NAME = re.compile(r'\bPV_[A-Z0-9_]+\b')


def sources():
    return sorted(glob.glob(os.path.join(PKG, 'csrc', '*'))) + [os.path.join(REPO, 'include', 'plenum_verify.h')]


def logical_lines(path):
    with open(path) as fh:
        return fh.read().replace('\\\n', ' ').split('\n')


def condition_names(paths):
    """PV_* names in #if / #ifdef / #ifndef / #elif conditions (defined(...) included) -> where"""
    found = {}
    for path in paths:
        for no, line in enumerate(logical_lines(path), 1):
            m = DIRECTIVE.match(line)
            if m:
                for name in NAME.findall(m.group(2).split('//')[0]):
                    found.setdefault(name, '{}:{}'.format(os.path.basename(path), no))
    return found


def default_pairs(paths):
    """PV_* names with an `#ifndef X` / `#define X` default (comment lines may sit between) -> where"""
    found = {}
    for path in paths:
        lines = logical_lines(path)
        for no, line in enumerate(lines):
            m = re.match(r'^\s*#\s*ifndef\s+(PV_[A-Z0-9_]+)\b', line)
            if not m:
                continue
            k = no + 1
            while k < len(lines) and (not lines[k].strip() or lines[k].strip().startswith('//')):
                k += 1
            if k < len(lines) and re.match(r'^\s*#\s*define\s+{}\b'.format(m.group(1)), lines[k]):
                found.setdefault(m.group(1), '{}:{}'.format(os.path.basename(path), no + 1))
    return found


def test_conditions_test_only_the_allowed_names():
    found = condition_names(sources())
    extra = {n: w for n, w in found.items() if n not in ALLOWED}
    assert not extra, 'compile-time switches outside the allow-list: {}'.format(extra)
    gone = sorted(set(ALLOWED) - set(found))
    assert not gone, 'allow-list entries that no condition tests any more: {}'.format(gone)


def test_no_default_for_a_name_outside_the_allow_list():
    pairs = default_pairs(sources())
    assert pairs, 'the scan found no #ifndef / #define default at all'
    extra = {n: w for n, w in pairs.items() if n not in ALLOWED}
    assert not extra, '#ifndef / #define defaults outside the allow-list: {}'.format(extra)
