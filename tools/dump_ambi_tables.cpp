// Writes what the compiled reference holds at run time of its ambisonic tables, as JSON on stdout: the seven upsampler
// matrices (AmbiScale::FirstOrderUp .. FourthOrder2DUp), the three scale tables (FromFuMa, FromSN3D, FromN3D) and the four
// index tables (AmbiIndex::FromFuMa, FromFuMa2D, FromACN, FromACN2D).  tools/make_ambi_tables.py packs the JSON into
// tests/golden/ambi_tables.npz, the fixture of tests/test_ambi_sources_host.py and tests/test_gpu_ambi_sources_bridge.py.
// Includes the reference's header by path and links the reference build's object that defines the matrices; not part of
// build().  From the repository root, after `make -C oracle ref` (REF: where the reference's sources lie):
//
//   g++ -std=gnu++20 -O1 -w -Ioracle/refcfg -I$REF -I$REF/include -I$REF/common -I$REF/gsl/include -I$REF/core \
//       -o oracle/_ref/dump_ambi_tables tools/dump_ambi_tables.cpp oracle/_ref/obj/core/ambidefs.cpp.o
//   oracle/_ref/dump_ambi_tables | python tools/make_ambi_tables.py tests/golden/ambi_tables.npz
#include <cstdio>

#include "core/ambidefs.h"

namespace {

bool first = true;

void Key(const char *name)
{
    std::printf("%s\"%s\": ", first ? "" : ",\n", name);
    first = false;
}

template<typename Rows>
void Matrix(const char *name, const Rows &rows)
{
    Key(name);
    std::printf("[");
    bool firstRow = true;
    for(const auto &row : rows)
    {
        std::printf("%s[", firstRow ? "" : ", ");
        firstRow = false;
        bool firstCol = true;
        for(const float v : row) { std::printf("%s%.9g", firstCol ? "" : ", ", double(v)); firstCol = false; }
        std::printf("]");
    }
    std::printf("]");
}

template<typename Row>
void Floats(const char *name, const Row &row)
{
    Key(name);
    std::printf("[");
    bool firstCol = true;
    for(const float v : row) { std::printf("%s%.9g", firstCol ? "" : ", ", double(v)); firstCol = false; }
    std::printf("]");
}

template<typename Row>
void Indices(const char *name, const Row &row)
{
    Key(name);
    std::printf("[");
    bool firstCol = true;
    for(const auto v : row) { std::printf("%s%u", firstCol ? "" : ", ", unsigned(v.c_val)); firstCol = false; }
    std::printf("]");
}

} // namespace

int main()
{
    std::printf("{\n");
    Matrix("FirstOrderUp", AmbiScale::FirstOrderUp);
    Matrix("FirstOrder2DUp", AmbiScale::FirstOrder2DUp);
    Matrix("SecondOrderUp", AmbiScale::SecondOrderUp);
    Matrix("SecondOrder2DUp", AmbiScale::SecondOrder2DUp);
    Matrix("ThirdOrderUp", AmbiScale::ThirdOrderUp);
    Matrix("ThirdOrder2DUp", AmbiScale::ThirdOrder2DUp);
    Matrix("FourthOrder2DUp", AmbiScale::FourthOrder2DUp);
    Floats("FromFuMa", AmbiScale::FromFuMa);
    Floats("FromSN3D", AmbiScale::FromSN3D);
    Floats("FromN3D", AmbiScale::FromN3D);
    Indices("IndexFromFuMa", AmbiIndex::FromFuMa);
    Indices("IndexFromFuMa2D", AmbiIndex::FromFuMa2D);
    Indices("IndexFromACN", AmbiIndex::FromACN);
    Indices("IndexFromACN2D", AmbiIndex::FromACN2D);
    std::printf("\n}\n");
    return 0;
}
