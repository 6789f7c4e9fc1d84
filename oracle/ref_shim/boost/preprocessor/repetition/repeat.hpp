// Stand-in for BOOST_PP_REPEAT (public macro name only; oracle/ref_shim/README.md): the one count the shader table uses, 4.
#pragma once
#define BOOST_PP_REPEAT(count, macro, data) BOOST_PP_REPEAT_STAND_IN(count, macro, data)
#define BOOST_PP_REPEAT_STAND_IN(count, macro, data) BOOST_PP_REPEAT_STAND_IN_##count(macro, data)
#define BOOST_PP_REPEAT_STAND_IN_4(macro, data) macro(2, 0, data) macro(2, 1, data) macro(2, 2, data) macro(2, 3, data)
