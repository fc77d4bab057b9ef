// Drop-in replacement for the reference's src/saca.rs (23 lines): same public items, same
// asserts, the engine call goes to libsuffix_array_amd.so instead of cdivsufsort.
// Not compiled in this repository's CI (no Rust toolchain on the build image); kept minimal
// so that review suffices.  Build: add `println!("cargo:rustc-link-lib=dylib=suffix_array_amd");`
// to a build.rs (and `cargo:rustc-link-search=native=<dir of the .so>`), drop the
// `cdivsufsort` dependency from Cargo.toml.

/// Maximum length of the input string.
pub const MAX_LENGTH: usize = std::i32::MAX as usize;

extern "C" {
    // include/suffix_array_amd.h: same signature as libdivsufsort's `divsufsort`
    fn sa_amd_divsufsort(t: *const u8, sa: *mut i32, n: i32) -> i32;
    // include/suffix_array_amd.h: the LCP array (an extension; uncompiled like the rest of this file)
    fn sa_amd_lcp(t: *const u8, n: i32, sa: *const u32, lcp: *mut u32) -> i32;
    fn sa_amd_saca_u8_lcp(t: *const u8, sa: *mut u32, n: i32, lcp: *mut u32) -> i32;
}

/// Wrapper of the underlying suffix array construction algorithm.
pub fn saca(s: &[u8], sa: &mut [u32]) {
    assert!(s.len() <= MAX_LENGTH);
    assert_eq!(s.len() + 1, sa.len());

    sa[0] = s.len() as u32;
    let ret = unsafe { sa_amd_divsufsort(s.as_ptr(), sa[1..].as_mut_ptr() as *mut i32, s.len() as i32) };
    assert_eq!(ret, 0, "suffix_array_amd engine failed with status {}", ret);
}

/// EXTENSION (not in the reference crate; its README's TODO "construct enhanced suffix array"):
/// the LCP array of `s` and its suffix array `sa` (layout of `saca`), computed on the GPU.
/// `lcp[0] == 0`; `lcp[i]` is the longest common prefix of the suffixes at `sa[i - 1]` and `sa[i]`.
/// `sa` must be the suffix array of `s` (not checked here); an entry beyond `s.len()` panics.
/// Uncompiled in this repository (no Rust toolchain on the build image).
pub fn lcp(s: &[u8], sa: &[u32]) -> Vec<u32> {
    assert!(s.len() <= MAX_LENGTH);
    assert_eq!(s.len() + 1, sa.len());

    let mut out = vec![0u32; s.len() + 1];
    let ret = unsafe { sa_amd_lcp(s.as_ptr(), s.len() as i32, sa.as_ptr(), out.as_mut_ptr()) };
    assert_eq!(ret, 0, "suffix_array_amd LCP failed with status {}", ret);
    out
}

/// The suffix array and its LCP array in one device round trip (the array is never uploaded).
pub fn saca_lcp(s: &[u8], sa: &mut [u32]) -> Vec<u32> {
    assert!(s.len() <= MAX_LENGTH);
    assert_eq!(s.len() + 1, sa.len());

    let mut out = vec![0u32; s.len() + 1];
    let ret = unsafe { sa_amd_saca_u8_lcp(s.as_ptr(), sa.as_mut_ptr(), s.len() as i32, out.as_mut_ptr()) };
    assert_eq!(ret, 0, "suffix_array_amd engine failed with status {}", ret);
    out
}
