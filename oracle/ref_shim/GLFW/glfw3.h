// GLFW/glfw3.h -- stand-in for the three GLFW / GL calls the reference's update() makes after the
// frame is computed (timer, texture upload).  They do nothing: oracle/ref_driver.cpp reads the
// frame from g_data.  Used only by oracle/Makefile.ref.
#ifndef ORACLE_REF_SHIM_GLFW3_H
#define ORACLE_REF_SHIM_GLFW3_H
enum { GL_TEXTURE_2D = 0, GL_RGBA = 0, GL_RGB = 0, GL_FLOAT = 0 };
inline double glfwGetTime() { return 0.0; }
inline void glBindTexture(int, unsigned int) {}
inline void glTexImage2D(int, int, int, int, int, int, int, int, const void *) {}
#endif
