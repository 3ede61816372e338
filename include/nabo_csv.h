/*
 * nabo_csv.h -- C ABI of the CSV table reader in libnabo_knn.so (MI355X, gfx950).
 *
 * Replaces the per-line `split` / `np.array(vec, dtype=float)` loop and the dict transpose of the reference's csv_to_h5
 * (nabo/_io.py:238-477): the BODY of a dense table of numbers (rows of `sep`-separated fields) is parsed on the device,
 * and its non-zero entries come back twice -- by row with ascending columns and by column with ascending rows.  Skipped
 * lines, the header line and what names mean are the caller's business (nabo_amd/_csv.py); this library sees data lines.
 * Same conventions as nabo_knn.h: 0 or a negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback for
 * the parse (NABO_E_NODEVICE without a device).  Every pointer is a host pointer, and every argument is checked on the
 * host before any device call.  The same bytes give the same arrays on every run, however they were fed.
 *
 * THE GRAMMAR
 *
 * A line ends at `\n`; the last line may lack its `\n`.  A blank is a space or a tab; a `\r` directly in front of a
 * `\n`, or at the end of the stream, counts as a blank.  An empty line (no byte, or that `\r` alone) is ignored when only
 * empty lines follow it up to the end of the stream, and an error anywhere else.  A line is split at EVERY separator
 * byte -- quotes do not protect one, as the reference's `split` does not -- and must have exactly n_cols + has_row_names
 * fields.  With has_row_names the first field is the row's name: any bytes, max_name of them at most, handed back raw.
 * Every other field is a value:
 *     value_kind 0 (float64)   blanks* [+-]? ( digits+ ( . digits* )? | . digits+ ) ( [eE] [+-]? digits+ )? blanks*
 *                              or, with an optional sign, `inf`, `infinity` or `nan` without regard to case
 *     value_kind 1 (int64)     blanks* [+-]? digits+ blanks*, in [-2^63, 2^63 - 1]
 * digits are ASCII 0-9.  Anything else is NABO_E_INVALID: an empty field, a quoted number, `NA`, hex, `1_0`, digits
 * outside ASCII.  Two departures from the reference follow from this: numpy 1.26 accepts `1_0` (as 10) and Unicode
 * digits.  A field of more than 4096 bytes is an error too.
 *
 * Errors.  The message begins `line N, field M:` for the LOWEST (line, field) of the stream that is wrong; N counts
 * from 1 at the first line fed, plus the first_line of nabo_csv_set_first_line; M counts the fields of the line from 1,
 * the name included.  A field in excess is judged in front of its own text (M = n_cols + has_row_names + 1), a missing
 * field is the one behind the last that is there.  On the device the lowest is found with a 64-bit atomicMin of
 * (byte offset << 8 | code), an integer minimum, so it is the same whatever the hardware does first.
 * After an error the handle accepts nothing but nabo_csv_free.
 *
 * WHICH FIELDS BECOME ENTRIES (the reference's _write_row_data, nabo/_io.py:429-437)
 *
 * The value is v.  With a threshold, v < null_thresh makes it 0 (int64 values are compared as doubles, as numpy
 * compares them); NaN < t is false, so a NaN stays.  The field is an entry iff v != 0: `0`, `-0.0`, `1e-400` and
 * `2e-324` are dropped, `nan` and `inf` are kept.  Rows and columns are 0-based; the row is the number of `\n` in front
 * of the field, the column the number of separators since the last of them (less one with row names).  Fewer than
 * 2^31 - 1 rows and columns, nnz below 2^32 - 1 (NABO_E_UNSUPPORTED otherwise).
 *
 * THE CONVERSION is bit-equal to C strtod / Python float() for every accepted field.  On the device (csv_number.h, the
 * same source the host tests run):
 *   - up to 19 significant digits are read into a uint64 w with the decimal exponent q, value = w * 10^q;
 *   - w = 0 or q < -342 is a signed zero (2^64 * 10^-343 is below half the smallest subnormal), q > 308 infinity;
 *   - Clinger's fast path when w <= 2^53 and |q| <= 22: one IEEE multiply or divide of two exact doubles;
 *   - otherwise the Eisel-Lemire step: the 64 x 64 -> 128-bit product of the normalised w with a table of truncated
 *     128-bit powers of five for q in [-342, 308], which the host builds once by exact multi-word integer arithmetic and
 *     uploads; subnormals, ties to even (possible only for q in [-4, 23]) and overflow to infinity are decided there.
 *     Proof obligation: the truncation of the table can hide a carry only when the low word of the product is all ones;
 *     for q in [-27, 55] the table entry is exact enough that it cannot.  So the device emits a value unless that word is
 *     all ones AND q lies outside [-27, 55].
 * Three kinds of field are DEFERRED, not errors: one whose rounding the step above does not prove; one with more than 19
 * significant digits (18 for int64); one longer than max_field bytes.  The device records where the field is, and the
 * host converts it with strtod / strtoll from the pinned text while the piece is still there (a long field is held to
 * the grammar first).  A deferred field that turns out to be zero or below the threshold is no entry.
 * A NaN has the bits 0x7FF8000000000000, with the sign bit for `-nan`.
 *
 * HOW IT RUNS
 *
 * feed buffers bytes in pinned host memory; once chunk_bytes are there, the bytes through the last separator or `\n`
 * are uploaded and parsed, and the unfinished field is carried to the front.  A line is far longer than a tile, so the
 * FIELD is the unit: it belongs to the tile (tile_bytes of text) in which its first byte lies, one workgroup per tile.
 * Each tile publishes (newlines, separators behind its last newline); a scan with that segmented operator gives every
 * tile its (row, column) base, and the host carries the base from piece to piece.  The parse kernel loads its tile and
 * max(max_field, max_name) bytes of look-ahead into LDS with 16-byte loads, builds the separator and `\n` bit masks,
 * and each lane converts the fields that start in its 64 bytes -- 32 entries at most (`1,1,1,...`), for which it owns 32
 * slots of a staging area.  A scan of the lanes' counts and a scan of the tiles' counts place the entries in file order,
 * which IS (row, column) order: row_ptr comes from the keys without a sort.  The by-column index is the transpose stage
 * of the Matrix Market reader, unchanged, with the entry's ordinal as its 4-byte payload and a gather of the values.
 *
 * Device memory.  With C the chunk size in use, P = max(C, 4097) + 1 and t = ceil(P / tile_bytes) tiles, a handle holds
 *     fixed(C) = P + 16 + t (131072 + 544) + 8 (P / (2 (n_cols + 1)) + 2) [with row names] + 16 (P / 5 + 2) + 10416 + 8 (n_cols + 1) + 256
 * bytes from nabo_csv_create on, and for `cap` entries -- the buffers grow by doubling -- 44 cap bytes at most, plus
 * 8 (n_rows + 1) and rocPRIM's temporary storage for the sort at finish.  A step that would pass mem_budget_bytes is
 * NABO_E_NOMEM.
 */
#ifndef NABO_CSV_H
#define NABO_CSV_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_csv nabo_csv;

/* A reader on `device`.  sep: the separator, one byte (0 .. 255), not `\n`, `\r` or a digit.  n_cols >= 1: the value
 * fields of a line.  has_row_names: the first field of a line is a name.  value_kind: 0 float64, 1 int64.
 * has_null_thresh, null_thresh: the threshold (not a NaN).  chunk_bytes: the text uploaded and parsed at a time; <= 0
 * means 16 MiB; values below 64 are raised to 64 and values above 256 MiB lowered to that.  mem_budget_bytes <= 0 means
 * three quarters of the device memory that is free at this call. */
int nabo_csv_create(int32_t device, int32_t sep, int64_t n_cols, int32_t has_row_names, int32_t value_kind, int32_t has_null_thresh,
                    double null_thresh, int64_t chunk_bytes, int64_t mem_budget_bytes, nabo_csv **out);

/* The lines in front of the first line fed (skipped lines, a header): added to N of every message.  Before the first feed. */
int nabo_csv_set_first_line(nabo_csv *h, int64_t first_line);

/* The next n bytes of the body, in ANY split: mid-field, one byte at a time, or all at once.  n = 0 is allowed. */
int nabo_csv_feed(nabo_csv *h, const void *bytes, int64_t n);

/* The end of the stream: parses the tail and builds both indexes.  Either output may be NULL.  Called once. */
int nabo_csv_finish(nabo_csv *h, int64_t *n_rows, int64_t *nnz);

/* After finish.  row_ptr int64[n_rows + 1], col int32[nnz], val 8 bytes[nnz] (double or int64 by value_kind): row r lists
 * col[row_ptr[r] .. row_ptr[r + 1]), strictly increasing.  An output may be NULL to leave it out. */
int nabo_csv_get_rows(nabo_csv *h, int64_t *row_ptr, int32_t *col, void *val);

/* After finish.  col_ptr int64[n_cols + 1], row int32[nnz], val 8 bytes[nnz]: column c lists row[col_ptr[c] ..
 * col_ptr[c + 1]), strictly increasing. */
int nabo_csv_get_cols(nabo_csv *h, int64_t *col_ptr, int32_t *row, void *val);

/* After finish, with has_row_names: name_off int64[n_rows + 1] and the raw bytes of every first field, name r =
 * name_bytes[name_off[r] .. name_off[r + 1]).  Call it with name_bytes NULL first: name_off[n_rows] is the size. */
int nabo_csv_get_row_names(nabo_csv *h, int64_t *name_off, void *name_bytes);

/* out[0] value fields seen, out[1] entries kept, out[2] fields converted on the device, out[3] fields deferred to the
 * host; out[0] = out[2] + out[3]. */
int nabo_csv_stats(nabo_csv *h, int64_t out[4]);

/* Device time in ms between HIP events, summed over the pieces: ms[0] upload of the text, ms[1] parse (count, bases,
 * conversion, placement, the host's deferred fields in between), ms[2] the indexes at finish (row_ptr, the transpose,
 * the gather), ms[3] the downloads so far; the number of pieces parsed. */
int nabo_csv_last_device_ms(nabo_csv *h, double ms[4], int64_t *n_chunks);

/* tile_bytes: the text one workgroup owns; max_field: the longest value field the device converts itself; max_name: the
 * longest row name. */
int nabo_csv_geometry(int32_t *tile_bytes, int32_t *max_field, int32_t *max_name);

void nabo_csv_free(nabo_csv *h);

#ifdef __cplusplus
}
#endif

#endif /* NABO_CSV_H */
