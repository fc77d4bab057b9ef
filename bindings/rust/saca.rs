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
    // include/suffix_array_amd.h: Lempel-Ziv factorisation (an extension; `sa` may be null: the array is then built on the device)
    #[allow(dead_code)]
    fn sa_amd_lpf(t: *const u8, n: i32, sa: *const u32, lpf: *mut u32, src: *mut u32) -> i32;
    #[allow(dead_code)]
    fn sa_amd_lz77(t: *const u8, n: i32, sa: *const u32, phrases: *mut u32, capacity: i64, count_out: *mut i64) -> i32;
    // include/suffix_array_amd.h: repeat finding (an extension; `sa` may be null: the array is then built on the device)
    fn sa_amd_repeat_spans_bound(n: i32, min_len: i32) -> i64;
    fn sa_amd_repeat_lengths(t: *const u8, n: i32, sa: *const u32, lr: *mut u32) -> i32;
    fn sa_amd_repeat_spans(t: *const u8, n: i32, sa: *const u32, min_len: i32, mode: i32, spans: *mut u32, capacity: i64,
                           count_out: *mut i64) -> i32;
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

/// EXTENSION (not in the reference crate): the longest-repeat array of `s`, computed on the GPU: `lr[p]` is the length of
/// the longest substring starting at `p` that also starts at some other position.  `sa`: the suffix array of `s` in the
/// layout of `saca`, or `None` to have it built on the device and never downloaded.
/// Uncompiled in this repository (no Rust toolchain on the build image).
pub fn repeat_lengths(s: &[u8], sa: Option<&[u32]>) -> Vec<u32> {
    assert!(s.len() <= MAX_LENGTH);
    if let Some(a) = sa {
        assert_eq!(s.len() + 1, a.len());
    }

    let mut out = vec![0u32; s.len()];
    let ptr = sa.map_or(std::ptr::null(), |a| a.as_ptr());
    let ret = unsafe { sa_amd_repeat_lengths(s.as_ptr(), s.len() as i32, ptr, out.as_mut_ptr()) };
    assert_eq!(ret, 0, "suffix_array_amd repeat lengths failed with status {}", ret);
    out
}

/// EXTENSION: the byte ranges of `s` that are copies, `[start, end)`, ascending, disjoint and not adjacent: every occurrence
/// of a substring of at least `min_len` bytes that occurs twice, or (`keep_first`) every window of `min_len` bytes equal
/// to an earlier one, so that the first copy of everything survives.  Only the spans come back from the device.
pub fn repeat_spans(s: &[u8], min_len: usize, keep_first: bool, sa: Option<&[u32]>) -> Vec<(u32, u32)> {
    assert!(s.len() <= MAX_LENGTH);
    assert!(min_len >= 1);
    if let Some(a) = sa {
        assert_eq!(s.len() + 1, a.len());
    }

    let k = std::cmp::min(min_len, MAX_LENGTH) as i32;
    let cap = unsafe { sa_amd_repeat_spans_bound(s.len() as i32, k) };
    let mut flat = vec![0u32; 2 * cap as usize];
    let mut count = 0i64;
    let ptr = sa.map_or(std::ptr::null(), |a| a.as_ptr());
    let ret = unsafe {
        sa_amd_repeat_spans(s.as_ptr(), s.len() as i32, ptr, k, keep_first as i32, flat.as_mut_ptr(), cap, &mut count)
    };
    assert_eq!(ret, 0, "suffix_array_amd repeat spans failed with status {}", ret);
    flat.chunks_exact(2).take(std::cmp::min(count, cap) as usize).map(|c| (c[0], c[1])).collect()
}
