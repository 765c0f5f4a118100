// ka_msa.hip -- rows of a finished alignment -> position maps (ka_msa.h): the sequence set, the host's row check, the
// upload and the one kernel that turns uploaded rows into col[] and res[].
#include "ka_ctx.h"
#include "ka_msa.h"

#define MSA_THREADS 256
#define MSA_WAVES (MSA_THREADS / 64)

// one wave per row (ka_msa_map_row): res[c] for every column of the row's res row, col[offs[s] + r] for every residue.  The rows
// are those of a batch of families, numbered flat (one alignment is a batch of one): a wave finds the family of its row
// (ka_fam_find), then the row's own start, width and place in res
__global__ __launch_bounds__(MSA_THREADS) void msa_maps_fam(KaMsaFamRows t, const uint8_t* rows, const long long* rowOff, const int* Wt, const int* cell,
                                                            int rowPad, int* col, int16_t* res)
{
        const int s = blockIdx.x * MSA_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (s >= t.S) return;
        const int f = ka_fam_find(t.firstSeq, t.nFam, s);
        const int W = Wt[f];
        if (W <= 0) return;                                      // (a family without rows in this batch)
        const int loc = s - t.firstSeq[f];
        ka_msa_map_row(rows + rowOff[f] + (long long)loc * (W + rowPad), W, W, t.lens[s], col + t.offs[s], res + cell[f] + (long long)loc * W, lane);
}

void ka_msa_launch_maps_fam(const KaMsaFamRows& t, const uint8_t* rows, const long long* rowOff, const int* W, const int* cell, int rowPad, int* col,
                            int16_t* res, hipStream_t s)
{
        msa_maps_fam<<<(t.S + MSA_WAVES - 1) / MSA_WAVES, MSA_THREADS, 0, s>>>(t, rows, rowOff, W, cell, rowPad, col, res);
}

int KaSeqSet::set(const char* who, int numseq, const int* l, int max_res, const char* why)
{
        const std::string w(who);
        N = numseq;
        lens.assign(l, l + numseq);
        offs.resize(numseq + 1);
        long long t = 0;
        for (int s = 0; s < numseq; s++) {
                if (l[s] < 0) return fail(w + ": negative sequence length");
                if (l[s] > max_res) return fail(w + ": sequence " + std::to_string(s) + " has " + std::to_string(l[s]) + " residues; " + why);
                offs[s] = (int)t;
                t += l[s];
                maxlen = std::max(maxlen, l[s]);
                if (t > INT32_MAX) return fail(w + ": more than 2^31 - 1 residues");
        }
        offs[numseq] = T = (int)t;
        return KA_OK;
}

int ka_msa_check_rows(const char* who, const KaSeqSet& q, const uint8_t* rows, long long stride, int alnlen)
{
        if (!rows) return fail(std::string(who) + ": no rows");
        if (alnlen <= 0 || stride < alnlen)
                return fail(std::string(who) + ": alignment width " + std::to_string(alnlen) + " does not fit row stride " + std::to_string(stride));
        for (int s = 0; s < q.N; s++) {
                const uint8_t* row = rows + (long long)s * stride;
                int n = 0;
                for (int c = 0; c < alnlen; c++) n += ka_msa_is_residue(row[c]);
                if (n != q.lens[s])
                        return fail(std::string(who) + ": row " + std::to_string(s) + " holds " + std::to_string(n) + " letters, its sequence " +
                                    std::to_string(q.lens[s]) + " (every alignment must hold the same sequences)");
        }
        return KA_OK;
}

int ka_msa_upload_rows(const KaSeqSet& q, uint8_t* dst, const uint8_t* rows, long long stride, int alnlen, hipStream_t s)
{
        HIPCHK(hipMemcpy2DAsync(dst, alnlen, rows, stride, alnlen, q.N, hipMemcpyHostToDevice, s));
        return KA_OK;
}
